// jpeg2png_amd — the marker segments of a baseline JPEG file, read in pure C before any device is chosen (include/jpeg2png_amd.h:
// "Reading a JPEG file"): the frame, the quantisation tables, the Huffman tables in the form the decode kernels look symbols up
// in, the component-to-table map, the restart interval and the byte range of the entropy-coded data.  The C twin of the
// Python package's jpeg_header(), which tests/test_decode_cpu.py holds it against.  No allocation, no global state; every
// read is checked against `size` first (tests/c/jpeg_parse_main.c runs it over prefixes and damaged copies under sanitizers).
// At the end, independent of all that: the reader of the EXIF Orientation tag (j2p_jpeg_orientation; tests/c/orientation_main.c).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "j2p_internal.h"

static const uint8_t kNaturalOfZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

static int refuse(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static int refuse(int code, const char *fmt, ...)
{
        char text[256];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof(text), fmt, ap);
        va_end(ap);
        j2p_set_last_error(text);
        return code;
}

// One DHT table: BITS (16 counts) and HUFFVAL (their sum symbols).  Codes are assigned in order of length, consecutive within a
// length, doubled from one length to the next; a table whose codes do not fit their length is refused, as libjpeg refuses it.
static int huffman_table(const uint8_t bits[16], const uint8_t *vals, unsigned nvals, int dc, j2p_huff_decode *t)
{
        memset(t, 0, sizeof(*t));
        memcpy(t->vals, vals, nvals);
        unsigned code = 0, k = 0;
        for(unsigned length = 1; length <= 16; length++) {
                const unsigned n = bits[length - 1];
                t->maxcode[length] = -1;
                t->valoff[length] = (int32_t)k - (int32_t)code;
                for(unsigned i = 0; i < n; i++, k++, code++) {
                        if(code >= (1u << length)) { return refuse(J2P_EFORMAT, "jpeg: a Huffman table's codes do not fit their lengths"); }
                        if(dc && vals[k] > 15) { return refuse(J2P_EFORMAT, "jpeg: a DC Huffman table holds category %u", vals[k]); }
                        if(length <= 8) {
                                // every 8-bit window that begins with this code
                                const unsigned first = code << (8 - length), count = 1u << (8 - length);
                                for(unsigned w = 0; w < count; w++) { t->look[first + w] = (uint16_t)((length << 8) | vals[k]); }
                        }
                }
                if(n) { t->maxcode[length] = (int32_t)code - 1; }
                code <<= 1;
        }
        t->defined = 1;
        return J2P_OK;
}

static unsigned be16(const uint8_t *p) { return ((unsigned)p[0] << 8) | p[1]; }
static unsigned ceil_div(unsigned a, unsigned b) { return (a + b - 1) / b; }

int j2p_jpeg_parse_full(const uint8_t *file, size_t size, j2p_jpeg_parsed *out)
{
        if(!file || !out) { return refuse(J2P_EINVAL, "NULL argument"); }
        memset(out, 0, sizeof(*out));
        j2p_jpeg_info *info = &out->info;
        if(size < 4 || file[0] != 0xff || file[1] != 0xd8) { return refuse(J2P_EFORMAT, "jpeg: not a JPEG file (no SOI marker)"); }
        int have_frame = 0;
        unsigned frame_quant[3] = {0, 0, 0};
        size_t pos = 2;
        for(;;) {
                if(pos + 2 > size) { return refuse(J2P_EFORMAT, "jpeg: the file ends before its scan"); }
                if(file[pos] != 0xff) { return refuse(J2P_EFORMAT, "jpeg: no marker at byte %zu", pos); }
                const unsigned marker = file[pos + 1];
                if(marker == 0xff) {            // a fill byte
                        pos++;
                        continue;
                }
                pos += 2;
                if(marker == 0x01 || (marker >= 0xd0 && marker <= 0xd8)) { continue; }  // TEM, RSTn, SOI: no segment
                if(marker == 0xd9) { return refuse(J2P_EFORMAT, "jpeg: EOI before the scan"); }
                if(pos + 2 > size) { return refuse(J2P_EFORMAT, "jpeg: truncated segment"); }
                const size_t length = be16(file + pos);
                if(length < 2 || length > size - pos) { return refuse(J2P_EFORMAT, "jpeg: truncated segment (marker FF%02X)", marker); }
                const uint8_t *body = file + pos + 2;
                const size_t n = length - 2;
                pos += length;
                if(marker == 0xdb) {                    // DQT: one or more tables, 8 or 16 bits an entry, zigzag order
                        size_t at = 0;
                        while(at < n) {
                                const unsigned precision = body[at] >> 4, slot = body[at] & 15;
                                at++;
                                if(precision > 1 || slot > 3) { return refuse(J2P_EFORMAT, "jpeg: invalid DQT segment"); }
                                const size_t bytes = precision ? 128 : 64;
                                if(bytes > n - at) { return refuse(J2P_EFORMAT, "jpeg: truncated segment (DQT)"); }
                                for(unsigned k = 0; k < 64; k++) {
                                        out->quant[slot][kNaturalOfZigzag[k]] = (uint16_t)(precision ? be16(body + at + 2 * k) : body[at + k]);
                                }
                                at += bytes;
                                out->quant_defined |= 1u << slot;
                        }
                } else if(marker == 0xc4) {             // DHT: one or more tables
                        size_t at = 0;
                        while(at < n) {
                                const unsigned cls = body[at] >> 4, slot = body[at] & 15;
                                at++;
                                if(cls > 1 || slot > 3) { return refuse(J2P_EFORMAT, "jpeg: invalid DHT segment"); }
                                if(16 > n - at) { return refuse(J2P_EFORMAT, "jpeg: truncated segment (DHT)"); }
                                unsigned count = 0;
                                for(unsigned k = 0; k < 16; k++) { count += body[at + k]; }
                                if(count > 256 || count > n - at - 16) { return refuse(J2P_EFORMAT, "jpeg: truncated segment (DHT)"); }
                                const int rc = huffman_table(body + at, body + at + 16, count, cls == 0, cls ? &out->ac[slot] : &out->dc[slot]);
                                if(rc != J2P_OK) { return rc; }
                                at += 16 + count;
                        }
                } else if(marker == 0xc0 || marker == 0xc1) {   // SOF0 / SOF1: Huffman coding, sequential
                        if(have_frame) { return refuse(J2P_EFORMAT, "jpeg: a second frame header"); }
                        if(n < 6) { return refuse(J2P_EFORMAT, "jpeg: truncated segment (SOF)"); }
                        if(body[0] == 12 || body[0] == 16) { return refuse(J2P_ENOTSUP, "jpeg: %u-bit samples (8-bit files are read)", body[0]); }
                        if(body[0] != 8) { return refuse(J2P_EFORMAT, "jpeg: %u-bit samples", body[0]); }
                        const unsigned nc = body[5];
                        if(nc == 0 || n != 6 + 3 * (size_t)nc) { return refuse(J2P_EFORMAT, "jpeg: invalid SOF segment"); }
                        if(nc != 1 && nc != 3) { return refuse(J2P_ENOTSUP, "jpeg: %u components (1 and 3 are read)", nc); }
                        info->height = be16(body + 1);
                        info->width = be16(body + 3);
                        if(info->width == 0) { return refuse(J2P_EFORMAT, "jpeg: invalid SOF segment (no width)"); }
                        if(info->height == 0) { return refuse(J2P_ENOTSUP, "jpeg: the height comes in a DNL segment"); }
                        info->ncomp = nc;
                        info->extended = marker == 0xc1;
                        for(unsigned c = 0; c < nc; c++) {
                                j2p_jpeg_component *k = &info->comp[c];
                                k->id = body[6 + 3 * c];
                                k->h_samp_factor = body[7 + 3 * c] >> 4;
                                k->v_samp_factor = body[7 + 3 * c] & 15;
                                frame_quant[c] = body[8 + 3 * c];
                                if(k->h_samp_factor < 1 || k->h_samp_factor > 4 || k->v_samp_factor < 1 || k->v_samp_factor > 4 || frame_quant[c] > 3) {
                                        return refuse(J2P_EFORMAT, "jpeg: invalid SOF segment (component %u)", c);
                                }
                        }
                        have_frame = 1;
                } else if(marker >= 0xc0 && marker <= 0xcf) {   // every other coding process, and DAC
                        static const char *const what[16] = {0, 0, "progressive", "lossless", 0, "hierarchical", "hierarchical", "hierarchical",
                                                             "reserved", "arithmetic", "arithmetic", "arithmetic", "arithmetic", "arithmetic", "arithmetic",
                                                             "arithmetic"};
                        return refuse(J2P_ENOTSUP, "jpeg: %s coding (marker FF%02X); baseline Huffman files are read", what[marker - 0xc0], marker);
                } else if(marker == 0xdd) {             // DRI
                        if(n != 2) { return refuse(J2P_EFORMAT, "jpeg: invalid DRI segment"); }
                        info->restart_interval = be16(body);
                } else if(marker == 0xdc) {
                        return refuse(J2P_ENOTSUP, "jpeg: a DNL segment");
                } else if(marker == 0xde || marker == 0xdf) {
                        return refuse(J2P_ENOTSUP, "jpeg: hierarchical coding (marker FF%02X)", marker);
                } else if(marker == 0xda) {             // SOS: the header ends here
                        if(!have_frame) { return refuse(J2P_EFORMAT, "jpeg: no SOF segment before SOS"); }
                        if(n < 1 || n != 4 + 2 * (size_t)body[0]) { return refuse(J2P_EFORMAT, "jpeg: invalid SOS segment"); }
                        const unsigned ns = body[0];
                        if(ns == 0 || ns > info->ncomp) { return refuse(J2P_EFORMAT, "jpeg: invalid SOS segment (%u components)", ns); }
                        if(ns != info->ncomp) { return refuse(J2P_ENOTSUP, "jpeg: several scans (the first holds %u of %u components)", ns, info->ncomp); }
                        for(unsigned c = 0; c < ns; c++) {
                                j2p_jpeg_component *k = &info->comp[c];
                                int known = 0;
                                for(unsigned o = 0; o < ns; o++) { known |= body[1 + 2 * c] == info->comp[o].id; }
                                if(!known) { return refuse(J2P_EFORMAT, "jpeg: the scan names component %u, the frame has none", body[1 + 2 * c]); }
                                if(body[1 + 2 * c] != k->id) { return refuse(J2P_ENOTSUP, "jpeg: the scan's components are not in the frame's order"); }
                                k->dc_slot = body[2 + 2 * c] >> 4;
                                k->ac_slot = body[2 + 2 * c] & 15;
                                if(k->dc_slot > 3 || k->ac_slot > 3) { return refuse(J2P_EFORMAT, "jpeg: invalid SOS segment (table slot)"); }
                        }
                        const uint8_t *tail = body + 1 + 2 * ns;
                        if(tail[0] != 0 || tail[1] != 63 || tail[2] != 0) {
                                return refuse(J2P_EFORMAT, "jpeg: a sequential scan with Ss %u, Se %u, Ah/Al %02X", tail[0], tail[1], tail[2]);
                        }
                        break;
                }
                // (APPn, COM and everything else with a length: skipped)
        }
        // the tables the scan names
        for(unsigned c = 0; c < info->ncomp; c++) {
                j2p_jpeg_component *k = &info->comp[c];
                k->quant_slot = frame_quant[c];
                if(!(out->quant_defined >> k->quant_slot & 1)) { return refuse(J2P_EFORMAT, "jpeg: component %u: quantisation table %u is missing", c, k->quant_slot); }
                if(!out->dc[k->dc_slot].defined) { return refuse(J2P_EFORMAT, "jpeg: component %u: DC Huffman table %u is missing", c, k->dc_slot); }
                if(!out->ac[k->ac_slot].defined) { return refuse(J2P_EFORMAT, "jpeg: component %u: AC Huffman table %u is missing", c, k->ac_slot); }
                memcpy(k->quant, out->quant[k->quant_slot], sizeof(k->quant));
        }
        // the grids: one component is coded block by block over its own grid, whatever sampling factors the frame states
        unsigned hmax = 1, vmax = 1;
        for(unsigned c = 0; c < info->ncomp; c++) {
                if(info->comp[c].h_samp_factor > hmax) { hmax = info->comp[c].h_samp_factor; }
                if(info->comp[c].v_samp_factor > vmax) { vmax = info->comp[c].v_samp_factor; }
        }
        info->blocks_per_mcu = 0;
        for(unsigned c = 0; c < info->ncomp; c++) {
                j2p_jpeg_component *k = &info->comp[c];
                k->blocks_w = ceil_div(ceil_div(info->width * k->h_samp_factor, hmax), 8);
                k->blocks_h = ceil_div(ceil_div(info->height * k->v_samp_factor, vmax), 8);
                k->w_samp = hmax / k->h_samp_factor;
                k->h_samp = vmax / k->v_samp_factor;
                info->blocks_per_mcu += info->ncomp == 1 ? 1 : k->h_samp_factor * k->v_samp_factor;
        }
        if(info->blocks_per_mcu > 10) { return refuse(J2P_EFORMAT, "jpeg: %u blocks in an MCU (10 at most)", info->blocks_per_mcu); }
        info->mcus_w = info->ncomp == 1 ? info->comp[0].blocks_w : ceil_div(info->width, 8 * hmax);
        info->mcus_h = info->ncomp == 1 ? info->comp[0].blocks_h : ceil_div(info->height, 8 * vmax);
        const unsigned long long mcus = (unsigned long long)info->mcus_w * info->mcus_h;
        info->intervals = info->restart_interval ? (unsigned)((mcus + info->restart_interval - 1) / info->restart_interval) : 1;
        // the entropy-coded data: up to the first marker that is neither a stuffed FF (FF 00), a fill byte (FF FF) nor RSTn
        info->scan_begin = pos;
        size_t end = pos;
        for(;;) {
                const uint8_t *ff = end < size ? memchr(file + end, 0xff, size - end) : NULL;
                if(!ff || (size_t)(ff - file) + 1 >= size) { return refuse(J2P_EFORMAT, "jpeg: the file ends inside its scan"); }
                end = (size_t)(ff - file);
                const unsigned next = file[end + 1];
                if(next == 0 || (next >= 0xd0 && next <= 0xd7)) {
                        end += 2;
                } else if(next == 0xff) {
                        end += 1;
                } else {
                        break;
                }
        }
        info->scan_end = end;
        // a block is at least two symbols, so at least two bits, and a restart marker two bytes: data that cannot hold what the
        // frame promises is truncated, whatever sizes the frame claims (nothing is ever allocated for such a file)
        {
                const unsigned long long bytes = end - info->scan_begin, blocks = mcus * info->blocks_per_mcu;
                if(bytes * 8 < 2 * blocks || info->intervals - 1 > bytes / 2) {
                        return refuse(J2P_EFORMAT, "jpeg: %llu bytes of data cannot hold the frame's %llu blocks in %u restart intervals", bytes, blocks, info->intervals);
                }
        }
        // what follows the scan: EOI, perhaps behind segments that do no harm; anything at all after EOI
        pos = end;
        for(;;) {
                if(pos + 2 > size) { return refuse(J2P_EFORMAT, "jpeg: the file ends before EOI"); }
                if(file[pos] != 0xff) { return refuse(J2P_EFORMAT, "jpeg: no marker at byte %zu", pos); }
                const unsigned marker = file[pos + 1];
                if(marker == 0xff) {
                        pos++;
                        continue;
                }
                pos += 2;
                if(marker == 0xd9) { break; }
                if(marker == 0xdc) { return refuse(J2P_ENOTSUP, "jpeg: a DNL segment"); }
                if(marker == 0xda) { return refuse(J2P_ENOTSUP, "jpeg: several scans"); }
                if(marker == 0x01 || (marker >= 0xd0 && marker <= 0xd8)) { return refuse(J2P_EFORMAT, "jpeg: marker FF%02X behind the scan", marker); }
                if(pos + 2 > size || be16(file + pos) < 2 || be16(file + pos) > size - pos) { return refuse(J2P_EFORMAT, "jpeg: truncated segment (marker FF%02X)", marker); }
                pos += be16(file + pos);
        }
        return J2P_OK;
}

int j2p_jpeg_parse(const uint8_t *file, size_t size, j2p_jpeg_info *info)
{
        if(!info) { return refuse(J2P_EINVAL, "NULL argument"); }
        j2p_jpeg_parsed parsed;
        const int rc = j2p_jpeg_parse_full(file, size, &parsed);
        if(rc == J2P_OK) {
                *info = parsed.info;
        } else {
                memset(info, 0, sizeof(*info));
        }
        return rc;
}

// ---- the EXIF Orientation tag (include/jpeg2png_amd.h: "Upright output") ----
// 16 / 32 bits of a TIFF structure in its byte order
static unsigned tiff16(const uint8_t *p, int big) { return big ? ((unsigned)p[0] << 8) | p[1] : ((unsigned)p[1] << 8) | p[0]; }
static unsigned long tiff32(const uint8_t *p, int big)
{
        return big ? ((unsigned long)p[0] << 24) | ((unsigned long)p[1] << 16) | ((unsigned long)p[2] << 8) | p[3]
                   : ((unsigned long)p[3] << 24) | ((unsigned long)p[2] << 16) | ((unsigned long)p[1] << 8) | p[0];
}

// the tag of one TIFF structure of n bytes (what follows "Exif\0\0" in its segment), 1 where it has none that counts
static unsigned tiff_orientation(const uint8_t *t, size_t n)
{
        if(n < 8) { return 1; }
        int big;
        if(t[0] == 'M' && t[1] == 'M') { big = 1; }
        else if(t[0] == 'I' && t[1] == 'I') { big = 0; }
        else { return 1; }
        if(tiff16(t + 2, big) != 42) { return 1; }
        const unsigned long ifd = tiff32(t + 4, big);
        if(ifd > n - 2) { return 1; }                   // (n >= 8: no wrap)
        const unsigned entries = tiff16(t + ifd, big);
        if((size_t)entries * 12 > n - 2 - ifd) { return 1; }     // an entry count that overruns the segment: a damaged structure
        for(unsigned k = 0; k < entries; k++) {
                const uint8_t *e = t + ifd + 2 + 12 * (size_t)k;
                if(tiff16(e, big) != 0x0112) { continue; }
                if(tiff16(e + 2, big) != 3 || tiff32(e + 4, big) != 1) { return 1; }      // SHORT, one value
                const unsigned v = tiff16(e + 8, big);
                return v >= 1 && v <= 8 ? v : 1;
        }
        return 1;
}

int j2p_jpeg_orientation(const uint8_t *file, size_t size, unsigned *orientation)
{
        if(!file || !orientation) { return refuse(J2P_EINVAL, "NULL argument"); }
        *orientation = 1;
        if(size < 4 || file[0] != 0xff || file[1] != 0xd8) { return J2P_OK; }
        size_t pos = 2;
        for(;;) {
                if(pos + 2 > size || file[pos] != 0xff) { return J2P_OK; }
                const unsigned marker = file[pos + 1];
                if(marker == 0xff) {            // a fill byte
                        pos++;
                        continue;
                }
                pos += 2;
                if(marker == 0x01 || (marker >= 0xd0 && marker <= 0xd8)) { continue; }  // TEM, RSTn, SOI: no segment
                if(marker == 0xd9 || marker == 0xda) { return J2P_OK; }                 // EOI, SOS: nothing is read beyond
                if(pos + 2 > size) { return J2P_OK; }
                const size_t length = be16(file + pos);
                if(length < 2 || length > size - pos) { return J2P_OK; }
                const uint8_t *body = file + pos + 2;
                const size_t n = length - 2;
                pos += length;
                if(marker == 0xe1 && n >= 6 && memcmp(body, "Exif\0\0", 6) == 0) {
                        *orientation = tiff_orientation(body + 6, n - 6);
                        return J2P_OK;
                }
        }
}
