// jpeg2png_amd — gfx950 device code of the table estimator (j2p_samples_histogram): the histogram of the step-1 coefficient
// magnitudes of a channel's 8-bit samples.  The definition is include/jpeg2png_amd.h, "Estimated tables"; the load, the transpose
// and the DCT pass are the ones sample input uses (j2p_dct.hip.h).  Bit-exactness rules: see j2p_kernels.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "j2p_dct.hip.h"

namespace j2p {

// The bins a workgroup keeps in LDS: all 1024 of the DC — a block's DC is 8 * (mean - 128), anywhere in the range — and the
// first kHistAcBins of each of the 63 other frequencies, whose values beyond that are a strong edge's and rare.  32-bit words:
// a workgroup cannot count 2^32 values.  36352 bytes, with the transposes' 13312 three workgroups a CU.
constexpr int kHistBins = 1024, kHistAcBins = 128;
constexpr int kHistLdsWords = kHistBins + 63 * kHistAcBins;
// the workgroups of a launch: each flushes up to kHistLdsWords global adds, so no more of them than keep every CU busy
constexpr unsigned kHistMaxWorkgroups = 512;

__device__ __forceinline__ int hist_lds_word(int j, unsigned m) { return j == 0 ? (int)m : kHistBins + (j - 1) * kHistAcBins + (int)m; }

// ---------------------------------------------------------------------------
// hist[j * 1024 + m] += the number of counted blocks whose coefficient j (natural order) has magnitude m = |rint(dct8x8s)|;
// counts[0] += counted blocks, counts[1] += excluded blocks (a sample of 0 or 255).  blocks_w x block_rows COMPLETE blocks:
// the host passes w / 8 and h / 8, so no load leaves the samples and nothing is replicated.
// Mapping of k_samples_to_coefficients: one wavefront = 8 horizontally adjacent blocks, lane >> 3 the block, lane & 7 the
// row, and after the two passes lane (b, rr) holds coefficients rr * 8 + 0..7 of block b.  A workgroup's four wavefronts
// walk the groups of 8 blocks with the grid's stride and count
//   m = 0 and m = 1 (almost every high-frequency value) in 16 registers a lane, folded over the 8 lanes that share rr once,
//                   at the end;
//   m >= 2          by one LDS add each into the workgroup's bins above, or — an AC value of kHistAcBins or more — by a
//                   global add at once;
// and the workgroup's bins go to `hist` once, by one global add per bin that is not 0.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_samples_dct_histogram(const uint8_t *data, ptrdiff_t stride_y, ptrdiff_t stride_x, int wide,
                                                               unsigned blocks_w, unsigned block_rows, unsigned *hist,
                                                               unsigned long long *counts)
{
        __shared__ __attribute__((aligned(16))) float tp[4 * kTpWave];
        __shared__ unsigned bins[kHistLdsWords];
        for(int i = (int)threadIdx.x; i < kHistLdsWords; i += 256) { bins[i] = 0u; }
        __syncthreads();
        const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
        const int b = lane >> 3, rr = lane & 7;
        const unsigned groups_x = (blocks_w + 7) / 8;
        const unsigned groups = groups_x * block_rows;                  // (below 2^31: the host refuses larger planes)
        float *scratch = tp + wave * kTpWave;
        unsigned n0[8], n1[8];
#pragma unroll
        for(int u = 0; u < 8; u++) { n0[u] = n1[u] = 0u; }
        unsigned counted_blocks = 0, excluded_blocks = 0;
        // (whole wavefronts take every turn of the loop: the transposes need all 64 lanes)
#pragma nounroll
        for(unsigned grp = blockIdx.x * 4 + (unsigned)wave; grp < groups; grp += gridDim.x * 4) {
                const unsigned by = grp / groups_x, bx = (grp % groups_x) * 8 + (unsigned)b;
                const bool ok = bx < blocks_w;
                unsigned s[8];
#pragma unroll
                for(int u = 0; u < 8; u++) { s[u] = 128u; }
                if(ok) { load_samples8(data + (ptrdiff_t)(by * 8 + (unsigned)rr) * stride_y + (ptrdiff_t)bx * 8 * stride_x, stride_x, wide, s); }
                bool clipped = false;
#pragma unroll
                for(int u = 0; u < 8; u++) { clipped = clipped || s[u] == 0u || s[u] == 255u; }
                // a block's 8 lanes are one byte of the ballots
                const unsigned long long present = __ballot(ok), clip = __ballot(clipped);
                const bool counts_in = ok && ((clip >> (b * 8)) & 0xffull) == 0ull;
                unsigned long long any = clip | (clip >> 4);
                any |= any >> 2;
                any |= any >> 1;
                const unsigned nex = (unsigned)__popcll(any & 0x0101010101010101ull);
                excluded_blocks += nex;
                counted_blocks += (unsigned)__popcll(present & 0x0101010101010101ull) - nex;
                float v[8];
#pragma unroll
                for(int u = 0; u < 8; u++) { v[u] = (float)s[u] - 128.f; }
                transpose8(v, scratch, lane);
                fdct8(v);
                transpose8(v, scratch, lane);
                fdct8(v);
                if(counts_in) {
#pragma unroll
                        for(int u = 0; u < 8; u++) {
                                const int r = (int)rintf(v[u]);
                                unsigned m = (unsigned)(r < 0 ? -r : r);
                                m = m < (unsigned)kHistBins ? m : (unsigned)kHistBins - 1u;       // (never taken: m <= 1016)
                                n0[u] += m == 0u ? 1u : 0u;
                                n1[u] += m == 1u ? 1u : 0u;
                                if(m >= 2u) {
                                        const int j = rr * 8 + u;
                                        if(j == 0 || m < (unsigned)kHistAcBins) { atomicAdd(&bins[hist_lds_word(j, m)], 1u); }
                                        else { atomicAdd(&hist[j * kHistBins + (int)m], 1u); }
                                }
                        }
                }
        }
        // the 8 lanes with one rr counted the same 8 frequencies: fold them, and the four wavefronts through the bins
#pragma unroll
        for(int u = 0; u < 8; u++) {
#pragma unroll
                for(int off = 8; off < 64; off <<= 1) {
                        n0[u] += (unsigned)__shfl_xor((int)n0[u], off, 64);
                        n1[u] += (unsigned)__shfl_xor((int)n1[u], off, 64);
                }
                if(b == 0) {
                        if(n0[u]) { atomicAdd(&bins[hist_lds_word(rr * 8 + u, 0u)], n0[u]); }
                        if(n1[u]) { atomicAdd(&bins[hist_lds_word(rr * 8 + u, 1u)], n1[u]); }
                }
        }
        if(lane == 0) {
                if(counted_blocks) { atomicAdd(&counts[0], (unsigned long long)counted_blocks); }
                if(excluded_blocks) { atomicAdd(&counts[1], (unsigned long long)excluded_blocks); }
        }
        __syncthreads();
        for(int i = (int)threadIdx.x; i < kHistLdsWords; i += 256) {
                const unsigned n = bins[i];
                if(n) {
                        const int j = i < kHistBins ? 0 : 1 + (i - kHistBins) / kHistAcBins;
                        const int m = i < kHistBins ? i : (i - kHistBins) % kHistAcBins;
                        atomicAdd(&hist[j * kHistBins + m], n);
                }
        }
}

}  // namespace j2p
