// jpeg2png_amd — the Huffman table made for one image's symbol counts (include/jpeg2png_amd.h: "Optimised Huffman tables"), as
// IJG libjpeg 9d and later make it: plain C and no HIP, so that tests/c/huffman_main.c holds it against the Python restatement
// (tests/huffman_cases.py) and the sanitizers on the CPU.  Used by the codec unit (j2p_codec.hip) between the histogram's
// read-back and the coding launches.
#pragma once
#include <stdint.h>
#include <string.h>

// libjpeg's own search for the two rarest symbols starts from this value and is undefined beyond it
#define J2P_HUFF_COUNT_MAX 1000000000ull
// the longest code the tree may have BEFORE the lengths are limited to 16 (libjpeg's MAX_CLEN; it dies on a longer one)
#define J2P_HUFF_TREE_MAX 32

#define J2P_HUFF_OK 0
#define J2P_HUFF_COUNT 1        // a count above J2P_HUFF_COUNT_MAX
#define J2P_HUFF_DEPTH 2        // a code longer than J2P_HUFF_TREE_MAX bits before limiting (more than 5 million symbols in all)

typedef struct j2p_huff_table {
        uint8_t bits[16];       // BITS[1..16]: codes of each length
        uint8_t vals[256];      // HUFFVAL: the first nvals are the table's symbols, by count descending, then by value ascending
        unsigned nvals;
        unsigned longest;       // the longest code before limiting (above 16: the lengths were limited)
} j2p_huff_table;

// count[s]: how often symbol s is coded.  No symbol at all gives the empty table (nvals 0).
static inline int j2p_huff_build(const uint64_t count[256], j2p_huff_table *out)
{
        uint64_t freq[257];
        int codesize[257], others[257];
        unsigned bits[J2P_HUFF_TREE_MAX + 1] = {0};
        memset(out, 0, sizeof(*out));
        for(int i = 0; i < 256; i++) {
                if(count[i] > J2P_HUFF_COUNT_MAX) { return J2P_HUFF_COUNT; }
                freq[i] = count[i];
                if(count[i]) { out->vals[out->nvals++] = (uint8_t)i; }
        }
        if(out->nvals == 0) { return J2P_HUFF_OK; }
        freq[256] = 1;                  // the pseudo-symbol that keeps the all-ones code unused
        for(int i = 0; i <= 256; i++) {
                codesize[i] = 0;
                others[i] = -1;
        }
        for(;;) {
                // the two rarest of what is left; of equals the one with the LARGEST index
                int c1 = -1, c2 = -1;
                for(int i = 0; i <= 256; i++) {
                        if(freq[i] && (c1 < 0 || freq[i] <= freq[c1])) { c1 = i; }
                }
                for(int i = 0; i <= 256; i++) {
                        if(freq[i] && i != c1 && (c2 < 0 || freq[i] <= freq[c2])) { c2 = i; }
                }
                if(c2 < 0) { break; }
                freq[c1] += freq[c2];
                freq[c2] = 0;
                // everything below c1 and below c2 grows by a bit; c2's chain is hung behind c1's
                codesize[c1]++;
                while(others[c1] >= 0) {
                        c1 = others[c1];
                        codesize[c1]++;
                }
                others[c1] = c2;
                codesize[c2]++;
                while(others[c2] >= 0) {
                        c2 = others[c2];
                        codesize[c2]++;
                }
        }
        for(int i = 0; i <= 256; i++) {
                if(codesize[i] > J2P_HUFF_TREE_MAX) { return J2P_HUFF_DEPTH; }
                if((unsigned)codesize[i] > out->longest) { out->longest = (unsigned)codesize[i]; }
                if(codesize[i]) { bits[codesize[i]]++; }
        }
        // no code longer than 16: a pair of the longest goes — one takes its prefix, the other shares the prefix of a shorter code
        for(int i = J2P_HUFF_TREE_MAX; i > 16; i--) {
                while(bits[i] > 0) {
                        int j = i - 2;
                        while(j > 0 && bits[j] == 0) { j--; }
                        if(j == 0) { return J2P_HUFF_DEPTH; }   // (no tree gets here: libjpeg checks the same)
                        bits[i] -= 2;
                        bits[i - 1] += 1;
                        bits[j + 1] += 2;
                        bits[j] -= 1;
                }
        }
        // the pseudo-symbol leaves from the longest length
        int last = 16;
        while(bits[last] == 0) { last--; }
        bits[last]--;
        for(int i = 1; i <= 16; i++) { out->bits[i - 1] = (uint8_t)bits[i]; }
        // the symbols by count descending (vals is in value order now; the sort is stable)
        for(unsigned i = 1; i < out->nvals; i++) {
                const uint8_t s = out->vals[i];
                unsigned k = i;
                for(; k > 0 && count[out->vals[k - 1]] < count[s]; k--) { out->vals[k] = out->vals[k - 1]; }
                out->vals[k] = s;
        }
        return J2P_HUFF_OK;
}
