// jpeg2png_amd — the host's part of the PNG coder (include/jpeg2png_amd.h: "The PNG file", items 4 and 5): from one deflate block's
// symbol counts, as k_png_count leaves them, to its code lengths, its codes, its header's bits and its size.  Plain C and no HIP, so
// that tests/c/deflate_main.c holds it against the Python restatement (tests/png_cases.py) and the sanitizers on the CPU.  Used by the
// codec unit (j2p_codec.hip) between the counts' read-back and the packing launch.  Nothing here is quadratic in the alphabet: an image
// has hundreds of blocks.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define J2P_DEFLATE_SYMBOLS 286         // literals 0..255, EOB 256, lengths 257..285
#define J2P_DEFLATE_COUNTS 288          // what the device leaves per block: the 286 counts, then the block's two Adler-32 sums
#define J2P_DEFLATE_HEADER_MAX 520      // bytes: 17 + 19 * 3 bits, then at most 287 lengths of at most 7 + 7 bits
#define J2P_DEFLATE_ADLER 65521u

// RFC 1951 3.2.5: length symbol 257 + k stands for the lengths from base[k] on, with extra[k] further bits
// (constexpr for the HIP unit, whose kernels check their own length symbols against the table at compile time)
#ifdef __cplusplus
#define J2P_DEFLATE_TABLE static constexpr
#else
#define J2P_DEFLATE_TABLE static const
#endif
J2P_DEFLATE_TABLE uint16_t j2p_deflate_length_base[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                                          31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
J2P_DEFLATE_TABLE uint8_t j2p_deflate_length_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
J2P_DEFLATE_TABLE uint8_t j2p_deflate_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

typedef struct j2p_deflate_block {
        uint8_t lengths[J2P_DEFLATE_SYMBOLS];   // of the literal/length code; 0: the block has not got the symbol
        uint32_t code[J2P_DEFLATE_SYMBOLS];     // (length << 16) | the code with its FIRST bit lowest, as deflate's bit order wants it
        uint8_t cl_lengths[19];                 // of the code-length code
        unsigned longest;                       // the longest literal/length code before limiting (above 15: the lengths were limited)
        unsigned hlit, hclen, dist_length;      // the header's fields; dist_length 1: the block has a match
        unsigned header_bits;                   // bits of `header`, which are the block's first
        uint8_t header[J2P_DEFLATE_HEADER_MAX];
        uint64_t literals, matches;             // tokens by kind
        uint64_t bytes;                         // the block with what follows it: the empty stored block, or the last block's padding
} j2p_deflate_block;

static inline int j2p_deflate_compare(const void *a, const void *b)
{
        const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
        return x < y ? -1 : (x > y ? 1 : 0);
}

// Code lengths of the n <= 286 symbols from their counts, none above `limit` (15 or 7): Huffman's algorithm with two queues — the
// leaves by count ascending, the nodes in the order they were made; the two smallest heads are joined, a leaf before a node of the
// same weight — then, while a length above the limit is in use, a pair of the longest goes (one takes its prefix, the other shares
// the prefix of a shorter code), and the lengths are dealt out, shortest first, by count descending and then symbol value ascending.
// *longest: the deepest leaf before limiting.  One symbol in use gets one bit.
static inline void j2p_deflate_lengths(const uint32_t *count, unsigned n, unsigned limit, uint8_t *lengths, unsigned *longest)
{
        uint64_t key[J2P_DEFLATE_SYMBOLS], weight[2 * J2P_DEFLATE_SYMBOLS];
        unsigned parent[2 * J2P_DEFLATE_SYMBOLS], depth[2 * J2P_DEFLATE_SYMBOLS], bits[J2P_DEFLATE_SYMBOLS + 1];
        unsigned used = 0;
        memset(lengths, 0, n);
        for(unsigned s = 0; s < n; s++) {
                if(count[s]) { key[used++] = ((uint64_t)count[s] << 16) | s; }
        }
        *longest = used ? 1 : 0;
        if(used == 0) { return; }
        if(used == 1) {
                lengths[key[0] & 0xffffu] = 1;
                return;
        }
        qsort(key, used, sizeof(key[0]), j2p_deflate_compare);
        for(unsigned k = 0; k < used; k++) { weight[k] = key[k] >> 16; }
        unsigned leaf = 0, node = used, made = used;
        for(unsigned step = 0; step + 1 < used; step++) {
                unsigned pick[2];
                for(int k = 0; k < 2; k++) {
                        if(leaf < used && (node >= made || weight[leaf] <= weight[node])) { pick[k] = leaf++; }
                        else { pick[k] = node++; }
                }
                weight[made] = weight[pick[0]] + weight[pick[1]];
                parent[pick[0]] = parent[pick[1]] = made;
                made++;
        }
        memset(bits, 0, sizeof(bits));
        depth[made - 1] = 0;
        unsigned deepest = 0;
        for(unsigned k = made - 1; k-- > 0;) {
                depth[k] = depth[parent[k]] + 1;
                if(k < used) {
                        bits[depth[k]]++;
                        if(depth[k] > deepest) { deepest = depth[k]; }
                }
        }
        *longest = deepest;
        for(unsigned i = deepest; i > limit; i--) {
                while(bits[i] > 0) {
                        unsigned j = i - 2;
                        while(bits[j] == 0) { j--; }            // (ends above 0: 2^limit codes are more than the alphabet has symbols)
                        bits[i] -= 2;
                        bits[i - 1] += 1;
                        bits[j + 1] += 2;
                        bits[j] -= 1;
                }
        }
        for(unsigned k = 0; k < used; k++) { key[k] = ((uint64_t)(0xffffffffu - (uint32_t)(key[k] >> 16)) << 16) | (key[k] & 0xffffu); }
        qsort(key, used, sizeof(key[0]), j2p_deflate_compare);
        unsigned k = 0;
        for(unsigned len = 1; len <= limit; len++) {
                for(unsigned i = 0; i < bits[len]; i++) { lengths[key[k++] & 0xffffu] = (uint8_t)len; }
        }
}

// RFC 1951 3.2.2: code[s] = (length << 16) | the canonical code of symbol s bit-reversed (its first bit lowest); 0 without a length
static inline void j2p_deflate_codes(const uint8_t *lengths, unsigned n, uint32_t *code)
{
        unsigned per_length[16] = {0}, next[16] = {0};
        for(unsigned s = 0; s < n; s++) { per_length[lengths[s]]++; }
        per_length[0] = 0;
        for(unsigned len = 1, c = 0; len < 16; len++) {
                c = (c + per_length[len - 1]) << 1;
                next[len] = c;
        }
        for(unsigned s = 0; s < n; s++) {
                const unsigned len = lengths[s];
                code[s] = 0;
                if(len == 0) { continue; }
                unsigned c = next[len]++, r = 0;
                for(unsigned b = 0; b < len; b++) { r |= ((c >> b) & 1u) << (len - 1 - b); }
                code[s] = (len << 16) | r;
        }
}

// `n` bits of `v`, lowest first, behind the *at bits that `bytes` holds already
static inline void j2p_deflate_put(uint8_t *bytes, unsigned *at, uint32_t v, unsigned n)
{
        for(unsigned b = 0; b < n; b++, (*at)++) { bytes[*at >> 3] |= (uint8_t)(((v >> b) & 1u) << (*at & 7u)); }
}

// Everything the packing kernel needs of one block, from its counts (count[256], EOB, must be 1).  final: the stream's last block.
static inline void j2p_deflate_block_make(const uint32_t count[J2P_DEFLATE_SYMBOLS], int final, j2p_deflate_block *out)
{
        memset(out, 0, sizeof(*out));
        j2p_deflate_lengths(count, J2P_DEFLATE_SYMBOLS, 15, out->lengths, &out->longest);
        j2p_deflate_codes(out->lengths, J2P_DEFLATE_SYMBOLS, out->code);
        uint64_t bits = 0;
        unsigned top = 256;
        for(unsigned s = 0; s < J2P_DEFLATE_SYMBOLS; s++) {
                if(!count[s]) { continue; }
                top = s > top ? s : top;
                bits += (uint64_t)count[s] * out->lengths[s];
                if(s < 256) { out->literals += count[s]; }
                if(s > 256) {
                        out->matches += count[s];
                        bits += (uint64_t)count[s] * (j2p_deflate_length_extra[s - 257] + 1u);  // (and the one-bit distance code)
                }
        }
        out->hlit = top + 1 - 257;
        out->dist_length = out->matches ? 1 : 0;
        // the lengths as symbols of the code-length code: a run of zeros as 18s (11..138) while 11 or more are left, then one 17
        // (3..10) or up to two zeros; a run of another length as the length once, then 16s (3..6) while 3 or more are left, then the
        // length itself.  The distance code's one length ends the sequence and takes part in the runs.
        uint8_t seq[J2P_DEFLATE_SYMBOLS + 1], sym[J2P_DEFLATE_SYMBOLS + 1], extra[J2P_DEFLATE_SYMBOLS + 1];
        const unsigned nseq = 257 + out->hlit + 1;
        memcpy(seq, out->lengths, nseq - 1);
        seq[nseq - 1] = (uint8_t)out->dist_length;
        unsigned nsym = 0;
        for(unsigned i = 0; i < nseq;) {
                unsigned j = i;
                while(j < nseq && seq[j] == seq[i]) { j++; }
                unsigned n = j - i;
                if(seq[i] == 0) {
                        while(n >= 11) {
                                const unsigned r = n < 138 ? n : 138;
                                sym[nsym] = 18;
                                extra[nsym++] = (uint8_t)(r - 11);
                                n -= r;
                        }
                        if(n >= 3) {
                                sym[nsym] = 17;
                                extra[nsym++] = (uint8_t)(n - 3);
                                n = 0;
                        }
                } else {
                        sym[nsym] = seq[i];
                        extra[nsym++] = 0;
                        n--;
                        while(n >= 3) {
                                const unsigned r = n < 6 ? n : 6;
                                sym[nsym] = 16;
                                extra[nsym++] = (uint8_t)(r - 3);
                                n -= r;
                        }
                }
                for(; n > 0; n--) {
                        sym[nsym] = seq[i];
                        extra[nsym++] = 0;
                }
                i = j;
        }
        uint32_t cl_count[19] = {0}, cl_code[19];
        for(unsigned k = 0; k < nsym; k++) { cl_count[sym[k]]++; }
        unsigned cl_longest;
        j2p_deflate_lengths(cl_count, 19, 7, out->cl_lengths, &cl_longest);
        j2p_deflate_codes(out->cl_lengths, 19, cl_code);
        unsigned last = 3;
        for(unsigned k = 4; k < 19; k++) {
                if(out->cl_lengths[j2p_deflate_cl_order[k]]) { last = k; }
        }
        out->hclen = last + 1 - 4;
        unsigned at = 0;
        j2p_deflate_put(out->header, &at, final ? 1u : 0u, 1);
        j2p_deflate_put(out->header, &at, 2, 2);
        j2p_deflate_put(out->header, &at, out->hlit, 5);
        j2p_deflate_put(out->header, &at, 0, 5);
        j2p_deflate_put(out->header, &at, out->hclen, 4);
        for(unsigned k = 0; k < out->hclen + 4; k++) { j2p_deflate_put(out->header, &at, out->cl_lengths[j2p_deflate_cl_order[k]], 3); }
        for(unsigned k = 0; k < nsym; k++) {
                j2p_deflate_put(out->header, &at, cl_code[sym[k]] & 0xffffu, cl_code[sym[k]] >> 16);
                j2p_deflate_put(out->header, &at, extra[k], sym[k] == 16 ? 2 : (sym[k] == 17 ? 3 : (sym[k] == 18 ? 7 : 0)));
        }
        out->header_bits = at;
        bits += at;
        // behind a block that is not the last: an empty stored block — three zero bits, zeros up to the byte, 00 00 FF FF
        out->bytes = final ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4;
}

// Adler-32 of a stream from its blocks' sums: a block of n bytes d_0 .. d_(n-1) gives s1 = sum d_i and s2 = sum (n - i) * d_i, both
// mod 65521.  *a, *b: the checksum's halves so far (1 and 0 at the start), carried over the block.
static inline void j2p_deflate_adler_add(uint32_t *a, uint32_t *b, uint64_t n, uint32_t s1, uint32_t s2)
{
        *b = (uint32_t)((*b + (n % J2P_DEFLATE_ADLER) * *a + s2) % J2P_DEFLATE_ADLER);
        *a = (*a + s1) % J2P_DEFLATE_ADLER;
}

static inline uint32_t j2p_crc32(const uint8_t *data, size_t n)
{
        uint32_t c = 0xffffffffu;
        for(size_t i = 0; i < n; i++) {
                c ^= data[i];
                for(int k = 0; k < 8; k++) { c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u))); }
        }
        return ~c;
}
