// jpeg2png_amd — the marker segments of a baseline JPEG file, read in pure C before any device is chosen (include/jpeg2png_amd.h:
// "Reading a JPEG file"): the frame, the quantisation tables, the Huffman tables in the form the decode kernels look symbols up
// in, the component-to-table map, the restart interval and the byte range of the entropy-coded data.  The C twin of the
// Python package's jpeg_header(), which tests/test_decode_cpu.py holds it against.  No allocation, no global state; every
// read is checked against `size` first (tests/c/jpeg_parse_main.c runs it over prefixes and damaged copies under sanitizers).
// Behind it the parser of every scan of a progressive file ("Reading a progressive JPEG file": j2p_jpeg_parse_scans, held against
// tests/scan_decode_cases.py by tests/test_scan_decode_cpu.py and run under sanitizers by tests/c/jpeg_scans_main.c).
// At the end, independent of all that: the reader of the EXIF Orientation tag (j2p_jpeg_orientation; tests/c/orientation_main.c).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
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

// ---- every scan of a progressive file (include/jpeg2png_amd.h: "Reading a progressive JPEG file") ----
// the entropy-coded data from `pos` on: up to the first marker that is neither a stuffed FF, a fill byte nor RSTn; 0: the file ends first
static size_t scan_data_end(const uint8_t *file, size_t size, size_t pos)
{
        size_t end = pos;
        for(;;) {
                const uint8_t *ff = end < size ? memchr(file + end, 0xff, size - end) : NULL;
                if(!ff || (size_t)(ff - file) + 1 >= size) { return 0; }
                end = (size_t)(ff - file);
                const unsigned next = file[end + 1];
                if(next == 0 || (next >= 0xd0 && next <= 0xd7)) {
                        end += 2;
                } else if(next == 0xff) {
                        end += 1;
                } else {
                        return end;
                }
        }
}

// the first frame header's marker (C0..CF without C4, C8, CC), 0 where none is found in front of the first SOS
static unsigned frame_marker(const uint8_t *file, size_t size)
{
        if(size < 4 || file[0] != 0xff || file[1] != 0xd8) { return 0; }
        size_t pos = 2;
        for(;;) {
                if(pos + 2 > size || file[pos] != 0xff) { return 0; }
                const unsigned marker = file[pos + 1];
                if(marker == 0xff) {
                        pos++;
                        continue;
                }
                pos += 2;
                if(marker == 0x01 || (marker >= 0xd0 && marker <= 0xd8)) { continue; }
                if(marker == 0xd9 || marker == 0xda) { return 0; }
                if(marker >= 0xc0 && marker <= 0xcf && marker != 0xc4 && marker != 0xc8 && marker != 0xcc) { return marker; }
                if(pos + 2 > size || be16(file + pos) < 2 || be16(file + pos) > size - pos) { return 0; }
                pos += be16(file + pos);
        }
}

// a single-scan sequential file through the scans parser: the baseline parse, as one scan
static int sequential_as_scans(const uint8_t *file, size_t size, j2p_scans_parsed *out)
{
        const int rc = j2p_jpeg_parse_full(file, size, &out->base);
        if(rc != J2P_OK) { return rc; }
        const j2p_jpeg_info *f = &out->base.info;
        j2p_jpeg_scan *s = &out->scans.scan[0];
        out->scans.nscans = 1;
        out->scans.progressive = 0;
        s->ncomp = f->ncomp;
        for(unsigned c = 0; c < f->ncomp; c++) {
                s->comp[c] = c;
                s->dc_slot[c] = f->comp[c].dc_slot;
                s->ac_slot[c] = f->comp[c].ac_slot;
        }
        s->se = 63;
        s->restart_interval = f->restart_interval;
        s->intervals = f->intervals;
        s->begin = f->scan_begin;
        s->end = f->scan_end;
        return J2P_OK;
}

static int progressive_scans(const uint8_t *file, size_t size, j2p_scans_parsed *out)
{
        j2p_jpeg_info *info = &out->base.info;
        j2p_jpeg_scans *scans = &out->scans;
        scans->progressive = 1;
        int have_frame = 0;
        unsigned frame_quant[3] = {0, 0, 0};
        unsigned restart = 0;                   // the interval in force
        int dc_now[4] = {-1, -1, -1, -1}, ac_now[4] = {-1, -1, -1, -1};        // [slot] the pool's table in force, -1: none yet
        int dc_named[3] = {0, 0, 0}, ac_named[3] = {0, 0, 0};
        signed char last_al[3][64];             // [component][coefficient] the Al of the last scan that covered it, -1: none has
        memset(last_al, -1, sizeof(last_al));
        unsigned hmax = 1, vmax = 1;
        size_t pos = 2;
        for(;;) {
                if(pos + 2 > size) { return refuse(J2P_EFORMAT, scans->nscans ? "jpeg: the file ends before EOI" : "jpeg: the file ends before its scan"); }
                if(file[pos] != 0xff) { return refuse(J2P_EFORMAT, "jpeg: no marker at byte %zu", pos); }
                const unsigned marker = file[pos + 1];
                if(marker == 0xff) {            // a fill byte
                        pos++;
                        continue;
                }
                pos += 2;
                if(marker == 0xd9) {
                        if(!scans->nscans) { return refuse(J2P_EFORMAT, "jpeg: EOI before the scan"); }
                        break;
                }
                if(marker == 0x01 || (marker >= 0xd0 && marker <= 0xd8)) {
                        if(scans->nscans) { return refuse(J2P_EFORMAT, "jpeg: marker FF%02X behind the scan", marker); }
                        continue;
                }
                if(pos + 2 > size) { return refuse(J2P_EFORMAT, "jpeg: truncated segment"); }
                const size_t length = be16(file + pos);
                if(length < 2 || length > size - pos) { return refuse(J2P_EFORMAT, "jpeg: truncated segment (marker FF%02X)", marker); }
                const uint8_t *body = file + pos + 2;
                const size_t n = length - 2;
                pos += length;
                if(marker == 0xdb) {
                        if(scans->nscans) { return refuse(J2P_ENOTSUP, "jpeg: a DQT segment behind the first scan"); }
                        size_t at = 0;
                        while(at < n) {
                                const unsigned precision = body[at] >> 4, slot = body[at] & 15;
                                at++;
                                if(precision > 1 || slot > 3) { return refuse(J2P_EFORMAT, "jpeg: invalid DQT segment"); }
                                const size_t bytes = precision ? 128 : 64;
                                if(bytes > n - at) { return refuse(J2P_EFORMAT, "jpeg: truncated segment (DQT)"); }
                                for(unsigned k = 0; k < 64; k++) {
                                        out->base.quant[slot][kNaturalOfZigzag[k]] = (uint16_t)(precision ? be16(body + at + 2 * k) : body[at + k]);
                                }
                                at += bytes;
                                out->base.quant_defined |= 1u << slot;
                        }
                } else if(marker == 0xc4) {
                        size_t at = 0;
                        while(at < n) {
                                const unsigned cls = body[at] >> 4, slot = body[at] & 15;
                                at++;
                                if(cls > 1 || slot > 3) { return refuse(J2P_EFORMAT, "jpeg: invalid DHT segment"); }
                                if(16 > n - at) { return refuse(J2P_EFORMAT, "jpeg: truncated segment (DHT)"); }
                                unsigned count = 0;
                                for(unsigned k = 0; k < 16; k++) { count += body[at + k]; }
                                if(count > 256 || count > n - at - 16) { return refuse(J2P_EFORMAT, "jpeg: truncated segment (DHT)"); }
                                if(out->ntables >= J2P_SCAN_TABLES_MAX) { return refuse(J2P_ENOTSUP, "jpeg: more than %u Huffman table definitions", J2P_SCAN_TABLES_MAX); }
                                const int rc = huffman_table(body + at, body + at + 16, count, cls == 0, &out->pool[out->ntables]);
                                if(rc != J2P_OK) { return rc; }
                                (cls ? ac_now : dc_now)[slot] = (int)out->ntables++;
                                at += 16 + count;
                        }
                } else if(marker == 0xc2) {
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
                        for(unsigned c = 0; c < nc; c++) {
                                j2p_jpeg_component *k = &info->comp[c];
                                k->id = body[6 + 3 * c];
                                k->h_samp_factor = body[7 + 3 * c] >> 4;
                                k->v_samp_factor = body[7 + 3 * c] & 15;
                                frame_quant[c] = body[8 + 3 * c];
                                if(k->h_samp_factor < 1 || k->h_samp_factor > 4 || k->v_samp_factor < 1 || k->v_samp_factor > 4 || frame_quant[c] > 3) {
                                        return refuse(J2P_EFORMAT, "jpeg: invalid SOF segment (component %u)", c);
                                }
                                if(k->h_samp_factor > hmax) { hmax = k->h_samp_factor; }
                                if(k->v_samp_factor > vmax) { vmax = k->v_samp_factor; }
                        }
                        // the grids, as the baseline parser lays them out
                        info->blocks_per_mcu = 0;
                        for(unsigned c = 0; c < nc; c++) {
                                j2p_jpeg_component *k = &info->comp[c];
                                k->blocks_w = ceil_div(ceil_div(info->width * k->h_samp_factor, hmax), 8);
                                k->blocks_h = ceil_div(ceil_div(info->height * k->v_samp_factor, vmax), 8);
                                k->w_samp = hmax / k->h_samp_factor;
                                k->h_samp = vmax / k->v_samp_factor;
                                info->blocks_per_mcu += nc == 1 ? 1 : k->h_samp_factor * k->v_samp_factor;
                        }
                        if(info->blocks_per_mcu > 10) { return refuse(J2P_EFORMAT, "jpeg: %u blocks in an MCU (10 at most)", info->blocks_per_mcu); }
                        info->mcus_w = nc == 1 ? info->comp[0].blocks_w : ceil_div(info->width, 8 * hmax);
                        info->mcus_h = nc == 1 ? info->comp[0].blocks_h : ceil_div(info->height, 8 * vmax);
                        have_frame = 1;
                } else if(marker >= 0xc0 && marker <= 0xcf) {
                        if(have_frame) { return refuse(J2P_EFORMAT, "jpeg: a second frame header"); }
                        return refuse(J2P_ENOTSUP, "jpeg: marker FF%02X in a progressive file", marker);
                } else if(marker == 0xdd) {
                        if(n != 2) { return refuse(J2P_EFORMAT, "jpeg: invalid DRI segment"); }
                        restart = be16(body);
                } else if(marker == 0xdc) {
                        return refuse(J2P_ENOTSUP, "jpeg: a DNL segment");
                } else if(marker == 0xde || marker == 0xdf) {
                        return refuse(J2P_ENOTSUP, "jpeg: hierarchical coding (marker FF%02X)", marker);
                } else if(marker == 0xda) {
                        if(!have_frame) { return refuse(J2P_EFORMAT, "jpeg: no SOF segment before SOS"); }
                        if(n < 1 || n != 4 + 2 * (size_t)body[0]) { return refuse(J2P_EFORMAT, "jpeg: invalid SOS segment"); }
                        const unsigned ns = body[0];
                        if(ns == 0 || ns > info->ncomp) { return refuse(J2P_EFORMAT, "jpeg: invalid SOS segment (%u components)", ns); }
                        if(scans->nscans >= J2P_DECODE_SCANS_MAX) { return refuse(J2P_ENOTSUP, "jpeg: more than %u scans", J2P_DECODE_SCANS_MAX); }
                        j2p_jpeg_scan *s = &scans->scan[scans->nscans];
                        memset(s, 0, sizeof(*s));
                        const uint8_t *tail = body + 1 + 2 * ns;
                        s->ncomp = ns;
                        s->ss = tail[0];
                        s->se = tail[1];
                        s->ah = tail[2] >> 4;
                        s->al = tail[2] & 15;
                        for(unsigned c = 0; c < ns; c++) {
                                unsigned which = 3;
                                for(unsigned o = 0; o < info->ncomp; o++) {
                                        if(body[1 + 2 * c] == info->comp[o].id) { which = o; }
                                }
                                if(which == 3) { return refuse(J2P_EFORMAT, "jpeg: the scan names component %u, the frame has none", body[1 + 2 * c]); }
                                if(c && which <= s->comp[c - 1]) { return refuse(J2P_ENOTSUP, "jpeg: the scan's components are not in the frame's order"); }
                                s->comp[c] = which;
                                s->dc_slot[c] = body[2 + 2 * c] >> 4;
                                s->ac_slot[c] = body[2 + 2 * c] & 15;
                                if(s->dc_slot[c] > 3 || s->ac_slot[c] > 3) { return refuse(J2P_EFORMAT, "jpeg: invalid SOS segment (table slot)"); }
                        }
                        // the progression (T.81 G.1.1.1.1, and what libjpeg warns about)
                        if(s->ss == 0 ? s->se != 0 : (ns != 1 || s->se < s->ss || s->se > 63)) {
                                return refuse(J2P_EFORMAT, "jpeg: bogus progression: Ss %u, Se %u in a scan of %u components", s->ss, s->se, ns);
                        }
                        if(s->al > 13 || (s->ah != 0 && s->ah != s->al + 1)) { return refuse(J2P_EFORMAT, "jpeg: bogus progression: Ah %u, Al %u", s->ah, s->al); }
                        unsigned long long blocks = 0, units = 0;
                        unsigned per_mcu = 0;
                        for(unsigned c = 0; c < ns; c++) {
                                const unsigned o = s->comp[c];
                                const j2p_jpeg_component *k = &info->comp[o];
                                if(s->ss && last_al[o][0] < 0) { return refuse(J2P_EFORMAT, "jpeg: bogus progression: an AC scan of component %u before its DC scan", o); }
                                for(unsigned i = s->ss; i <= s->se; i++) {
                                        const unsigned expected = last_al[o][i] < 0 ? 0 : (unsigned)last_al[o][i];
                                        if(s->ah != expected || (last_al[o][i] >= 0 && s->ah == 0)) {
                                                return refuse(J2P_EFORMAT, "jpeg: bogus progression: component %u, coefficient %u: Ah %u follows Al %d", o, i, s->ah, last_al[o][i]);
                                        }
                                        last_al[o][i] = (signed char)s->al;
                                }
                                // the tables in force
                                if(s->ss == 0 && s->ah == 0) {
                                        if(dc_now[s->dc_slot[c]] < 0) { return refuse(J2P_EFORMAT, "jpeg: component %u: DC Huffman table %u is missing", o, s->dc_slot[c]); }
                                        out->dc_table[scans->nscans][c] = (uint16_t)dc_now[s->dc_slot[c]];
                                        if(!dc_named[o]) {
                                                dc_named[o] = 1;
                                                info->comp[o].dc_slot = s->dc_slot[c];
                                        }
                                }
                                if(s->ss) {
                                        if(ac_now[s->ac_slot[c]] < 0) { return refuse(J2P_EFORMAT, "jpeg: component %u: AC Huffman table %u is missing", o, s->ac_slot[c]); }
                                        out->ac_table[scans->nscans] = (uint16_t)ac_now[s->ac_slot[c]];
                                        if(!ac_named[o]) {
                                                ac_named[o] = 1;
                                                info->comp[o].ac_slot = s->ac_slot[c];
                                        }
                                }
                                per_mcu += ns == 1 ? 1 : k->h_samp_factor * k->v_samp_factor;
                                if(ns == 1) { units = (unsigned long long)k->blocks_w * k->blocks_h; }
                        }
                        if(ns > 1) { units = (unsigned long long)info->mcus_w * info->mcus_h; }
                        if(per_mcu > 10) { return refuse(J2P_EFORMAT, "jpeg: %u blocks in an MCU (10 at most)", per_mcu); }
                        blocks = units * per_mcu;
                        s->restart_interval = restart;
                        s->intervals = restart ? (unsigned)((units + restart - 1) / restart) : 1;
                        s->begin = pos;
                        s->end = scan_data_end(file, size, pos);
                        if(s->end == 0) { return refuse(J2P_EFORMAT, "jpeg: the file ends inside its scan"); }
                        // what the data must hold at the least: a bit for every block of a DC scan, a bit for every 32767 blocks of an AC
                        // scan (one EOB run), two bytes for every restart marker — a claimed size alone makes nobody allocate
                        {
                                const unsigned long long bytes = s->end - s->begin;
                                const unsigned long long need = s->ss ? (blocks + 32766) / 32767 : blocks;
                                if(bytes * 8 < need || s->intervals - 1 > bytes / 2) {
                                        return refuse(J2P_EFORMAT, "jpeg: %llu bytes of data cannot hold the scan's %llu blocks in %u restart intervals", bytes, blocks, s->intervals);
                                }
                        }
                        if(scans->nscans == 0) {
                                info->scan_begin = s->begin;
                                info->restart_interval = restart;
                                for(unsigned c = 0; c < info->ncomp; c++) {
                                        j2p_jpeg_component *k = &info->comp[c];
                                        k->quant_slot = frame_quant[c];
                                        if(!(out->base.quant_defined >> k->quant_slot & 1)) {
                                                return refuse(J2P_EFORMAT, "jpeg: component %u: quantisation table %u is missing", c, k->quant_slot);
                                        }
                                        memcpy(k->quant, out->base.quant[k->quant_slot], sizeof(k->quant));
                                }
                        }
                        info->scan_end = s->end;
                        info->intervals += s->intervals;
                        scans->nscans++;
                        pos = s->end;
                }
                // (APPn, COM and everything else with a length: skipped)
        }
        return J2P_OK;
}

int j2p_jpeg_parse_scans_full(const uint8_t *file, size_t size, j2p_scans_parsed *out)
{
        if(!file || !out) { return refuse(J2P_EINVAL, "NULL argument"); }
        memset(&out->base, 0, sizeof(out->base));
        memset(&out->scans, 0, sizeof(out->scans));
        out->ntables = 0;
        if(size < 4 || file[0] != 0xff || file[1] != 0xd8) { return refuse(J2P_EFORMAT, "jpeg: not a JPEG file (no SOI marker)"); }
        return frame_marker(file, size) == 0xc2 ? progressive_scans(file, size, out) : sequential_as_scans(file, size, out);
}

// (the internal form is large — every table definition of the file — and lives in the caller's hands or, here, on the heap)
int j2p_jpeg_parse_scans(const uint8_t *file, size_t size, j2p_jpeg_info *info, j2p_jpeg_scans *scans)
{
        if(!info || !scans) { return refuse(J2P_EINVAL, "NULL argument"); }
        j2p_scans_parsed *parsed = file ? malloc(sizeof(*parsed)) : NULL;
        if(file && !parsed) { return refuse(J2P_ENOMEM, "out of memory"); }
        const int rc = file ? j2p_jpeg_parse_scans_full(file, size, parsed) : refuse(J2P_EINVAL, "NULL argument");
        if(rc == J2P_OK) {
                *info = parsed->base.info;
                *scans = parsed->scans;
        } else {
                memset(info, 0, sizeof(*info));
                memset(scans, 0, sizeof(*scans));
        }
        free(parsed);
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
