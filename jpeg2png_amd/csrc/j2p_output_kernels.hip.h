// jpeg2png_amd — gfx950 device code of the output stage: what turns solved planes into samples (k_to_samples), tensor
// elements (k_to_tensor, k_to_tensor_resized, k_filter_taps + k_to_tensor_filtered, and for several outputs in one call
// k_filter_taps_outputs + k_to_tensors_filtered) and quantised JPEG coefficients (k_quantise_blocks; from there to the
// entropy-coded file: j2p_codec_kernels.hip.h), and what lays an oriented solver's planes upright in front of any of them
// (k_upright_rows, k_upright_transpose).  A device translation
// unit of its own (j2p_output.hip), so that an edit here does not recompile the solver's kernels (j2p_kernels.hip.h), with
// which it shares only j2p_dct.hip.h.  Compiled with the same flags: -ffp-contract=off, no fast-math, correctly rounded `/`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "j2p_dct.hip.h"

namespace j2p {

// ---------------------------------------------------------------------------
// YCbCr -> RGB of the PNG writer (png.c:37-62) with the luma +128 fix-up of
// jpeg2png.c:156-159, cropped to the image size.  The reference evaluates the
// colour matrix in double, narrows to float for the clamp, scales by
// (1 << bits) / 256 in float and truncates to unsigned; the same here.
// out: one byte per sample (bits == 8) or two, big-endian (bits == 16).
// ---------------------------------------------------------------------------
__device__ __forceinline__ float clamp_sample(double v)
{
        const float x = (float)v;
        return (double)x > 255. ? 255.f : ((double)x < 0. ? 0.f : x);           // CLAMP(x, 0., 255.), png.c:15-17
}

// One pixel up to the clamp, for k_to_samples and k_to_tensor alike: put(k, x) gets the clamped float x of output channel k,
// from the solved Y, Cb, Cr.  NPLANE 3: RGB.  NPLANE 1: greyscale — the same writer with Cb = Cr = 0, where R = G = B exactly
// (yi + 0.0 and yi - 0.0 - 0.0 in double are yi), so the colour matrix is not evaluated and cbi / cri are not looked at.
template <int NPLANE, typename Put>
__device__ __forceinline__ void clamped_pixel(float y, float cbi, float cri, Put put)
{
        static_assert(NPLANE == 1 || NPLANE == 3, "greyscale or RGB");
        const float yi = (float)((double)y + 128.);                             // jpeg2png.c:158
        if constexpr(NPLANE == 3) {
                put(0, clamp_sample((double)yi + 1.402 * (double)cri));
                put(1, clamp_sample((double)yi - 0.34414 * (double)cbi - 0.71414 * (double)cri));
                put(2, clamp_sample((double)yi + 1.772 * (double)cbi));
        } else {
                put(0, clamp_sample((double)yi));
        }
}

// the sample(s) of one pixel as big-endian bytes: one byte each (bits == 8) or two (bits == 16)
template <int N>
__device__ __forceinline__ void store_samples(uint8_t *out, size_t i, const unsigned (&v)[N], unsigned bits)
{
        if(bits == 8) {
                uint8_t *o = out + i * N;
#pragma unroll
                for(int k = 0; k < N; k++) { o[k] = (uint8_t)(v[k] & 0xff); }
        } else {
                uint8_t *o = out + i * (2 * N);
#pragma unroll
                for(int k = 0; k < N; k++) { o[2 * k] = (uint8_t)((v[k] >> 8) & 0xff); o[2 * k + 1] = (uint8_t)(v[k] & 0xff); }
        }
}

// NPLANE 3: RGB.  NPLANE 1: greyscale, where cbp / crp are not read.  out: NPLANE samples per pixel.
template <int NPLANE>
__global__ __launch_bounds__(256) void k_to_samples(const float *yp, unsigned ys, const float *cbp, unsigned cbs, const float *crp,
                                                    unsigned crs, unsigned w, unsigned h, unsigned bits, uint8_t *out)
{
        const size_t n = (size_t)w * h;
        const float bitfactor = (float)((double)(1 << bits) / 256.);
        for(size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
                const unsigned x = (unsigned)(i % w), y = (unsigned)(i / w);
                const float yin = yp[(size_t)y * ys + x];
                float cbi = 0.f, cri = 0.f;                                      // (one plane: not looked at)
                if constexpr(NPLANE == 3) { cbi = cbp[(size_t)y * cbs + x]; cri = crp[(size_t)y * crs + x]; }
                unsigned v[NPLANE];
                clamped_pixel<NPLANE>(yin, cbi, cri, [&](int k, float x) { v[k] = (unsigned)(x * bitfactor); });
                store_samples(out, i, v, bits);
        }
}
// Instantiated explicitly: an implicit instantiation is emitted at the end of the code object, where the same instructions
// measured 2 us (5 %) slower per 4096x3072 image than k_to_rgb did from here (profiles/README.md: output_stage_refactor)
template __global__ void k_to_samples<3>(const float *, unsigned, const float *, unsigned, const float *, unsigned, unsigned, unsigned, unsigned, uint8_t *);
template __global__ void k_to_samples<1>(const float *, unsigned, const float *, unsigned, const float *, unsigned, unsigned, unsigned, unsigned, uint8_t *);

// ---------------------------------------------------------------------------
// Tensor output: the same conversion up to the clamp (png.c:37-47 with the luma +128 of jpeg2png.c:156-159), left in DEVICE
// memory as elements of a strided tensor — element (k, y, x) at data + k * stride_c + y * stride_y + x * stride_x, strides
// in elements.  Per channel k with the clamped float v_k:
//   u8                : (uint8_t)(unsigned)v_k — the 8-bit samples of k_to_samples;
//   f32 / f16 / bf16  : t = v_k * scale[k], then t = t + bias[k] — two separately rounded f32 operations (this file is
//                       compiled with -ffp-contract=off; never an fma, and no shortcut for scale 1 / bias 0: -0.f + 0.f is
//                       +0.f) — stored as it is (f32) or rounded to nearest even by the cast (f16, bf16: which instruction
//                       that is, is the compiler's choice).
// Indexed in 2-D, no division anywhere: blockIdx.x and the lane give the column, the wavefront of the workgroup and
// blockIdx.y the row, grid-stride over rows.  A lane converts 4 consecutive pixels of one row from ONE 16-byte load per
// plane: its first column is a multiple of 4, crops start at canvas column 0, every canvas row starts at a multiple of W
// floats with W a multiple of 8, and the planes themselves are carved from the solver's arena at multiples of 256
// bytes (Carver::take in j2p_solver.hip) — so every such load is aligned and, W being a multiple of 4, inside the canvas row even where the
// image ends inside the group.  A wavefront reads 1 KB of every plane's row.
// LAYOUT (chosen by the host, tensor_path in j2p_output.hip, the only place that knows the rule):
//   planar      (stride_x == 1): a lane's 4 elements of a channel go out as one 16 / 8 / 4-byte store (f32 / 16-bit / u8);
//   interleaved (stride_c == 1, stride_x == NPLANE): its 4 * NPLANE contiguous elements as NPLANE such stores;
//   generic     : one element per store, any strides.
// The first two are only launched where every such store is aligned to its width; the w % 4 pixels at the end of a row take
// the element stores in every layout.  Nothing but elements of the image is ever written.
// ---------------------------------------------------------------------------
constexpr int kDtypeU8 = 0, kDtypeF16 = 1, kDtypeBF16 = 2, kDtypeF32 = 3;                // J2P_DTYPE_* (checked in j2p_output.hip)
constexpr int kTensorGeneric = 0, kTensorPlanar = 1, kTensorInterleaved = 2;           // what j2p_debug_tensor_path reports

struct TensorOut {
        void *data;                                     // element (0, first row, 0)
        long long stride_c, stride_y, stride_x;         // in elements
        float scale[3], bias[3];
};

template <int DTYPE>
struct TensorElement {
        static_assert(DTYPE == kDtypeU8 || DTYPE == kDtypeF16 || DTYPE == kDtypeBF16 || DTYPE == kDtypeF32, "u8, f16, bf16 or f32");
        static constexpr int kBytes = DTYPE == kDtypeU8 ? 1 : (DTYPE == kDtypeF32 ? 4 : 2);
        using Raw = std::conditional_t<kBytes == 1, uint8_t, std::conditional_t<kBytes == 2, uint16_t, uint32_t>>;
        // the element's bits from the clamped float
        static __device__ __forceinline__ unsigned make(float v, float scale, float bias)
        {
                if constexpr(DTYPE == kDtypeU8) {
                        return (unsigned)(uint8_t)(unsigned)v;
                } else {
                        float t = v * scale;
                        t = t + bias;
                        if constexpr(DTYPE == kDtypeF32) { return __float_as_uint(t); }
                        else if constexpr(DTYPE == kDtypeF16) { return (unsigned)__builtin_bit_cast(uint16_t, (_Float16)t); }
                        else { return (unsigned)__builtin_bit_cast(uint16_t, (__bf16)t); }
                }
        }
};

// WORDS 32-bit words as one store: 16, 8 or 4 bytes
template <int WORDS>
__device__ __forceinline__ void store_words(void *p, const unsigned *v)
{
        static_assert(WORDS == 1 || WORDS == 2 || WORDS == 4, "4, 8 or 16 bytes");
        if constexpr(WORDS == 4) { *reinterpret_cast<uint4 *>(p) = make_uint4(v[0], v[1], v[2], v[3]); }
        else if constexpr(WORDS == 2) { *reinterpret_cast<uint2 *>(p) = make_uint2(v[0], v[1]); }
        else { *reinterpret_cast<unsigned *>(p) = v[0]; }
}

// the rows of one lane: columns [x0, x0 + npix).  FULL: npix is 4 — a loop of its own, so that the compiler sees all four loaded
// values used and keeps the 16-byte loads whole (with npix a run-time value in one loop it loads three floats and one)
template <int NPLANE, int DTYPE, int LAYOUT, bool FULL>
__device__ __forceinline__ void tensor_lane_rows(const float *yp, unsigned ys, const float *cbp, unsigned cbs, const float *crp, unsigned crs,
                                                 unsigned x0, unsigned npix, unsigned h, const TensorOut &o)
{
        using E = TensorElement<DTYPE>;
        using Raw = typename E::Raw;
        constexpr int kPerWord = 4 / E::kBytes;         // elements per 32-bit word
        constexpr int kWords = E::kBytes;               // words of one store of 4 elements: 16 / 8 / 4 bytes
        Raw *const data = static_cast<Raw *>(o.data);
        for(unsigned y = blockIdx.y * 4 + (threadIdx.x >> 6); y < h; y += gridDim.y * 4) {
                const float4 y4 = *reinterpret_cast<const float4 *>(yp + (size_t)y * ys + x0);
                const float yin[4] = {y4.x, y4.y, y4.z, y4.w};
                float4 cb4 = make_float4(0.f, 0.f, 0.f, 0.f), cr4 = cb4;                  // (one plane: not looked at)
                if constexpr(NPLANE == 3) {
                        cb4 = *reinterpret_cast<const float4 *>(cbp + (size_t)y * cbs + x0);
                        cr4 = *reinterpret_cast<const float4 *>(crp + (size_t)y * crs + x0);
                }
                const float cbin[4] = {cb4.x, cb4.y, cb4.z, cb4.w}, crin[4] = {cr4.x, cr4.y, cr4.z, cr4.w};
                float v[NPLANE][4];
#pragma unroll
                for(int p = 0; p < 4; p++) { clamped_pixel<NPLANE>(yin[p], cbin[p], crin[p], [&](int k, float x) { v[k][p] = x; }); }
                unsigned e[NPLANE][4];
#pragma unroll
                for(int k = 0; k < NPLANE; k++) {
#pragma unroll
                        for(int p = 0; p < 4; p++) { e[k][p] = E::make(v[k][p], o.scale[k], o.bias[k]); }
                }
                const long long row = (long long)y * o.stride_y;
                if constexpr(LAYOUT != kTensorGeneric && FULL) {
                        // the lane's elements in memory order, packed into words: NPLANE stores of kWords words
                        unsigned words[NPLANE * kWords];
#pragma unroll
                        for(int i = 0; i < NPLANE * kWords; i++) { words[i] = 0; }
#pragma unroll
                        for(int i = 0; i < NPLANE * 4; i++) {
                                const unsigned bits = LAYOUT == kTensorPlanar ? e[i / 4][i % 4] : e[i % NPLANE][i / NPLANE];
                                words[i / kPerWord] |= bits << (8 * E::kBytes * (i % kPerWord));
                        }
#pragma unroll
                        for(int j = 0; j < NPLANE; j++) {
                                Raw *dst = LAYOUT == kTensorPlanar ? data + (long long)j * o.stride_c + row + x0
                                                                   : data + row + (long long)x0 * NPLANE + j * 4;
                                store_words<kWords>(dst, words + j * kWords);
                        }
                } else {
#pragma unroll
                        for(int p = 0; p < 4; p++) {
                                if(FULL || (unsigned)p < npix) {
#pragma unroll
                                        for(int k = 0; k < NPLANE; k++) {
                                                data[(long long)k * o.stride_c + row + (long long)(x0 + p) * o.stride_x] = (Raw)e[k][p];
                                        }
                                }
                        }
                }
        }
}

template <int NPLANE, int DTYPE, int LAYOUT>
__global__ __launch_bounds__(256) void k_to_tensor(const float *yp, unsigned ys, const float *cbp, unsigned cbs, const float *crp,
                                                   unsigned crs, unsigned w, unsigned h, TensorOut o)
{
        static_assert(NPLANE == 1 || NPLANE == 3, "greyscale or RGB");
        static_assert(LAYOUT == kTensorGeneric || LAYOUT == kTensorPlanar || (LAYOUT == kTensorInterleaved && NPLANE == 3), "layout");
        const unsigned x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
        if(x0 >= w) { return; }                                                 // (no barrier in this kernel)
        if(w - x0 >= 4) { tensor_lane_rows<NPLANE, DTYPE, LAYOUT, true>(yp, ys, cbp, cbs, crp, crs, x0, 4, h, o); }
        else { tensor_lane_rows<NPLANE, DTYPE, kTensorGeneric, false>(yp, ys, cbp, cbs, crp, crs, x0, w - x0, h, o); }   // the row's last w % 4 pixels
}
// (explicit instantiations, as for k_to_samples; one plane has no interleaved layout: stride_x == 1 there, which is planar)
#define J2P_TENSOR_KERNEL(NPLANE, DTYPE, LAYOUT)                                                                                   \
        template __global__ void k_to_tensor<NPLANE, DTYPE, LAYOUT>(const float *, unsigned, const float *, unsigned, const float *, \
                                                                    unsigned, unsigned, unsigned, TensorOut);
#define J2P_TENSOR_KERNELS(DTYPE)                                                                                                  \
        J2P_TENSOR_KERNEL(3, DTYPE, kTensorGeneric) J2P_TENSOR_KERNEL(3, DTYPE, kTensorPlanar) J2P_TENSOR_KERNEL(3, DTYPE, kTensorInterleaved) \
        J2P_TENSOR_KERNEL(1, DTYPE, kTensorGeneric) J2P_TENSOR_KERNEL(1, DTYPE, kTensorPlanar)
J2P_TENSOR_KERNELS(kDtypeU8)
J2P_TENSOR_KERNELS(kDtypeF16)
J2P_TENSOR_KERNELS(kDtypeBF16)
J2P_TENSOR_KERNELS(kDtypeF32)
#undef J2P_TENSOR_KERNELS
#undef J2P_TENSOR_KERNEL

// ---------------------------------------------------------------------------
// Resized tensor output: the clamped floats v_k of a source rectangle (the box) of the image, area-resampled to out_w x
// out_h <= the box, as elements of the same strided tensor.  Every bit is defined (include/jpeg2png_amd.h):
//   taps of output column X, in integers: lo = X * box_w, hi = lo + box_w; source columns i = lo / out_w .. (hi - 1) / out_w
//   of the box with weights a_i = min(hi, (i + 1) * out_w) - max(lo, i * out_w); rows likewise with box_h, out_h, b_j.  An
//   axis that is not resized has one tap of weight 1: the host passes its taps in the units (1, 1) and no divisor;
//   r_j = 0.f; r_j = r_j + (float)a_i * v_k(box_x + i, box_y + j), i ascending;  acc = 0.f; acc = acc + (float)b_j * r_j,
//   j ascending;  m = acc [/ (float)box_w] [/ (float)box_h] (the IEEE quotients), m = min(m, 255.f), and TensorElement of m.
// Every operation rounded on its own (-ffp-contract=off, correctly rounded division, never a reciprocal).  The products
// X * box_w are formed in 64 bits (a zoomed canvas is wider than 65535); what the tap walk carries is the tap's offset
// i * out_w - lo, which lies in (-out_w, box_w) and fits an int.
// MAPPING: a wavefront owns `rows` consecutive output rows of a tile of lanes x slots output columns, column X0 + p * lanes +
// lane in slot p of its lane (neighbouring lanes: neighbouring columns, for the stores and for the LDS banks).  For every
// source row of those output rows' footprint, in order, it goes left to right through the row segment its tile covers in chunks of
// kResizeChunk columns: the lanes load the chunk with 16-byte loads (aligned DOWN to 4 floats: up to 3 columns left of the
// box and what is right of the segment in its last group are converted and never looked at; the group lies inside the canvas
// row as k_to_tensor's does), convert every pixel ONCE and stage the clamped channels in wave-private LDS; then every lane
// walks those taps of its columns that lie in the chunk.  Chunks ascend, so every r_j is summed in the order above
// whatever the tile and the chunk size are.  The LDS index is padded by one float per 32 (resize_lds_index): lanes read at a
// stride of box_w / out_w floats, and with the pad the strides 2, 4, 8, 16 touch 32 distinct banks per 32-lane half, as the
// four dword stores of the staging do (a lane's 4 floats are then no longer 16-byte aligned, but 4 conflict-free dword
// stores cost the LDS the cycles of one 16-byte store).  No workgroup barrier: the 4 wavefronts of a workgroup (one above
// the other in one tile, so that the source row two of them share is in L1 / L2 for the second) do not talk to each other.
// Where two consecutive output rows of a wavefront share a source row, the second starts from the same r_j (acc = 0.f + b *
// r_j): the row is read and converted once.  The loads of the next chunk are issued before the taps of this one are walked.
// The tile is the host's choice (resize_tile in j2p_output.hip): 256 columns and 8 rows where the output is large, down to
// 32 columns and one row where it is small, so that a small output of a large image still gives every SIMD a wavefront or
// two.
// Element stores and generic strides only: the output is small next to the source that is read.
// ---------------------------------------------------------------------------
constexpr int kResizeChunk = 512;                                // source columns staged at a time (a multiple of 256)
constexpr int kResizeSlots = 4;                                  // output columns per lane, at most
constexpr int kResizeLds = kResizeChunk + kResizeChunk / 32;     // floats per staged channel

struct ResizeGeom {
        unsigned box_x, box_y;
        unsigned tap_bw, tap_ow;        // the units of the x taps: (box_w, out_w), or (1, 1) where the axis is not resized
        unsigned tap_bh, tap_oh;
        unsigned qx, rx, qy, ry;        // tap_bw = qx * tap_ow + rx, tap_bh = qy * tap_oh + ry
        unsigned qlanes, rlanes;        // lanes * tap_bw = qlanes * tap_ow + rlanes
        unsigned out_w, out_h;
        float div_x, div_y;             // (float)box_w, (float)box_h; 0.f: axis not resized, no division
        unsigned lanes, slots;          // the tile: lanes (a power of two, 32 or 64) x slots (1..kResizeSlots) columns
        unsigned rows;                  // consecutive output rows per wavefront
};

__device__ __forceinline__ int resize_lds_index(int i) { return i + (i >> 5); }

// the taps of an output index of an axis: source indices [first, last] of the box, and rem with lo = first * ow + rem,
// 0 <= rem < ow — the first tap's offset first * ow - lo is -rem
struct ResizeTaps {
        int first, last, rem;
};
// last = (lo + bw - 1) / ow without a division: with bw = q * ow + r that is first + q + floor((rem + r - 1) / ow), and
// rem + r - 1 lies in [-1, 2 * ow - 2]
__device__ __forceinline__ ResizeTaps resize_taps_from(int first, int rem, unsigned q, unsigned r, unsigned ow)
{
        const int t = rem + (int)r - 1;
        ResizeTaps out;
        out.first = first;
        out.last = first + (int)q + (t >= (int)ow ? 1 : (t < 0 ? -1 : 0));
        out.rem = rem;
        return out;
}
// of index X, by a 64-bit division: once per wavefront and axis
__device__ __forceinline__ ResizeTaps resize_taps(unsigned X, unsigned bw, unsigned ow, unsigned q, unsigned r)
{
        const unsigned long long lo = (unsigned long long)X * bw, first = lo / ow;
        return resize_taps_from((int)first, (int)(lo - first * ow), q, r, ow);
}
// of the index `step` further on, where step * bw = qs * ow + rs
__device__ __forceinline__ ResizeTaps resize_taps_step(const ResizeTaps &t, unsigned qs, unsigned rs, unsigned q, unsigned r, unsigned ow)
{
        int first = t.first + (int)qs, rem = t.rem + (int)rs;           // (rem < 2 * ow)
        if(rem >= (int)ow) { rem -= (int)ow; first++; }
        return resize_taps_from(first, rem, q, r, ow);
}
// the weight of the tap at offset off = i * ow - lo: min(hi, (i + 1) * ow) - max(lo, i * ow), both taken relative to lo
__device__ __forceinline__ float resize_weight(int off, unsigned bw, unsigned ow)
{
        const int end = off + (int)ow;
        return (float)((end < (int)bw ? end : (int)bw) - (off > 0 ? off : 0));
}

template <int NPLANE, int DTYPE>
__global__ __launch_bounds__(256) void k_to_tensor_resized(const float *yp, unsigned ys, const float *cbp, unsigned cbs, const float *crp,
                                                           unsigned crs, ResizeGeom g, TensorOut o)
{
        static_assert(NPLANE == 1 || NPLANE == 3, "greyscale or RGB");
        static_assert(kResizeChunk % 256 == 0, "whole rounds of 64 lanes x 4 floats");
        constexpr int kRounds = kResizeChunk / 256;
        using E = TensorElement<DTYPE>;
        using Raw = typename E::Raw;
        __shared__ float stage[4][NPLANE][kResizeLds];
        const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
        const unsigned Yb = (blockIdx.y * 4 + (unsigned)wave) * g.rows;   // this wavefront's output rows: [Yb, Ye)
        if(Yb >= g.out_h) { return; }                                    // (no workgroup barrier in this kernel)
        const unsigned Ye = g.out_h - Yb < g.rows ? g.out_h : Yb + g.rows;
        float (*const lds)[kResizeLds] = stage[wave];
        const unsigned tile = g.lanes * g.slots;
        const unsigned X0 = blockIdx.x * tile;                           // (the grid has no tile beyond out_w)
        const unsigned ncol = g.out_w - X0 < tile ? g.out_w - X0 : tile;
        // the taps of the lane's columns X0 + p * lanes + lane: from the tile's first column by steps, no division per column
        // but one of 32 bits (lane * tap_bw < 64 * 2^18)
        const ResizeTaps t0 = resize_taps(X0, g.tap_bw, g.tap_ow, g.qx, g.rx);
        ResizeTaps tx[kResizeSlots];
        bool has[kResizeSlots];
        {
                const unsigned lb = (unsigned)lane * g.tap_bw, ql = lb / g.tap_ow;
                tx[0] = resize_taps_step(t0, ql, lb - ql * g.tap_ow, g.qx, g.rx, g.tap_ow);
        }
#pragma unroll
        for(int p = 0; p < kResizeSlots; p++) {
                if(p > 0) { tx[p] = resize_taps_step(tx[p - 1], g.qlanes, g.rlanes, g.qx, g.rx, g.tap_ow); }
                has[p] = (unsigned)p < g.slots && (unsigned)lane < g.lanes && (unsigned)p * g.lanes + (unsigned)lane < ncol;
        }
        // the tile's segment of a source row, in canvas columns: [c_begin, c_last], c_begin a multiple of 4
        const int c_last = (int)g.box_x + resize_taps(X0 + ncol - 1, g.tap_bw, g.tap_ow, g.qx, g.rx).last;
        const int c_begin = ((int)g.box_x + t0.first) & ~3;
        ResizeTaps ty = resize_taps(Yb, g.tap_bh, g.tap_oh, g.qy, g.ry);
        const int j_end = resize_taps(Ye - 1, g.tap_bh, g.tap_oh, g.qy, g.ry).last;        // the last source row of these output rows
        Raw *const data = static_cast<Raw *>(o.data);

        // the 16-byte loads of chunk c0 of source row j, into registers: issued one chunk ahead of their use
        float4 ld[kRounds][NPLANE];
#pragma unroll
        for(int u = 0; u < kRounds; u++) {
#pragma unroll
                for(int k = 0; k < NPLANE; k++) { ld[u][k] = make_float4(0.f, 0.f, 0.f, 0.f); }
        }
        const auto issue = [&](int j, int c0) {
                const size_t row = (size_t)g.box_y + (size_t)j;
#pragma unroll
                for(int u = 0; u < kRounds; u++) {
                        const int c = c0 + u * 256 + lane * 4;
                        if(c <= c_last) {
                                ld[u][0] = *reinterpret_cast<const float4 *>(yp + row * ys + c);
                                if constexpr(NPLANE == 3) {
                                        ld[u][1] = *reinterpret_cast<const float4 *>(cbp + row * cbs + c);
                                        ld[u][2] = *reinterpret_cast<const float4 *>(crp + row * crs + c);
                                }
                        }
                }
        };

        unsigned Y = Yb;
        float acc[kResizeSlots][NPLANE];
#pragma unroll
        for(int p = 0; p < kResizeSlots; p++) {
#pragma unroll
                for(int k = 0; k < NPLANE; k++) { acc[p][k] = 0.f; }
        }
        int offy = -ty.rem;                                              // source row j's offset j * tap_oh - lo of output row Y
        issue(ty.first, c_begin);
        for(int j = ty.first;; j++) {
                // r_j of every column of the lane: the row's chunks, left to right
                float r[kResizeSlots][NPLANE];
#pragma unroll
                for(int p = 0; p < kResizeSlots; p++) {
#pragma unroll
                        for(int k = 0; k < NPLANE; k++) { r[p][k] = 0.f; }
                }
                for(int c0 = c_begin; c0 <= c_last; c0 += kResizeChunk) {
#pragma unroll
                        for(int u = 0; u < kRounds; u++) {
                                const int at = u * 256 + lane * 4;
                                if(c0 + at <= c_last) {
                                        const float yin[4] = {ld[u][0].x, ld[u][0].y, ld[u][0].z, ld[u][0].w};
                                        const float4 cb4 = ld[u][NPLANE == 3 ? 1 : 0], cr4 = ld[u][NPLANE == 3 ? 2 : 0];   // (one plane: not looked at)
                                        const float cbin[4] = {cb4.x, cb4.y, cb4.z, cb4.w}, crin[4] = {cr4.x, cr4.y, cr4.z, cr4.w};
#pragma unroll
                                        for(int q = 0; q < 4; q++) {
                                                const int idx = resize_lds_index(at + q);
                                                clamped_pixel<NPLANE>(yin[q], cbin[q], crin[q], [&](int k, float x) { lds[k][idx] = x; });
                                        }
                                }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        // the next chunk's loads fly while this one's taps are walked
                        if(c0 + kResizeChunk <= c_last) { issue(j, c0 + kResizeChunk); }
                        else if(j < j_end) { issue(j + 1, c_begin); }
                        const int rel0 = c0 - (int)g.box_x;              // the chunk's first column relative to the box (>= -3)
#pragma unroll
                        for(int p = 0; p < kResizeSlots; p++) {
                                if(!has[p]) { continue; }
                                const int i0 = tx[p].first > rel0 ? tx[p].first : rel0;
                                const int i1 = tx[p].last < rel0 + kResizeChunk - 1 ? tx[p].last : rel0 + kResizeChunk - 1;
                                if(i0 > i1) { continue; }                // none of this column's taps in this chunk
                                int off = (i0 - tx[p].first) * (int)g.tap_ow - tx[p].rem;         // (< box_w + out_w)
                                for(int i = i0; i <= i1; i++, off += (int)g.tap_ow) {
                                        const float a = resize_weight(off, g.tap_bw, g.tap_ow);
                                        const int idx = resize_lds_index(i - rel0);
#pragma unroll
                                        for(int k = 0; k < NPLANE; k++) {
                                                const float t = a * lds[k][idx];
                                                r[p][k] = r[p][k] + t;
                                        }
                                }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();                 // the next chunk is staged over this one
                }
                // output row Y takes the row with its weight; where the row is Y's last, Y is finished, and the next output
                // row, if the row is its first (the one source row two output rows share), starts from the same r_j
                const float b = resize_weight(offy, g.tap_bh, g.tap_oh);
                offy += (int)g.tap_oh;
#pragma unroll
                for(int p = 0; p < kResizeSlots; p++) {
#pragma unroll
                        for(int k = 0; k < NPLANE; k++) {
                                const float t = b * r[p][k];
                                acc[p][k] = acc[p][k] + t;
                        }
                }
                if(j < ty.last) { continue; }
                const long long rowo = (long long)Y * o.stride_y;
#pragma unroll
                for(int p = 0; p < kResizeSlots; p++) {
                        if(!has[p]) { continue; }
                        const long long X = (long long)(X0 + (unsigned)p * g.lanes + (unsigned)lane);
#pragma unroll
                        for(int k = 0; k < NPLANE; k++) {
                                float m = acc[p][k];
                                if(g.div_x != 0.f) { m = m / g.div_x; }
                                if(g.div_y != 0.f) { m = m / g.div_y; }
                                m = m < 255.f ? m : 255.f;
                                data[(long long)k * o.stride_c + rowo + X * o.stride_x] = (Raw)E::make(m, o.scale[k], o.bias[k]);
                        }
                }
                if(++Y == Ye) { break; }
                ty = resize_taps_step(ty, g.qy, g.ry, g.qy, g.ry, g.tap_oh);
                offy = -ty.rem;
                const bool shared = ty.first == j;                      // (a resized axis has at least two taps: never also Y's last)
                const float b2 = shared ? resize_weight(offy, g.tap_bh, g.tap_oh) : 0.f;
                if(shared) { offy += (int)g.tap_oh; }
#pragma unroll
                for(int p = 0; p < kResizeSlots; p++) {
#pragma unroll
                        for(int k = 0; k < NPLANE; k++) {
                                const float t = b2 * r[p][k];
                                acc[p][k] = 0.f + t;                      // (not shared: 0.f + 0.f * r_j, which is +0.f: r_j is finite and not negative)
                        }
                }
        }
}
#define J2P_RESIZED_KERNELS(NPLANE)                                                                                                          \
        template __global__ void k_to_tensor_resized<NPLANE, kDtypeU8>(const float *, unsigned, const float *, unsigned, const float *, unsigned, ResizeGeom, TensorOut);   \
        template __global__ void k_to_tensor_resized<NPLANE, kDtypeF16>(const float *, unsigned, const float *, unsigned, const float *, unsigned, ResizeGeom, TensorOut);  \
        template __global__ void k_to_tensor_resized<NPLANE, kDtypeBF16>(const float *, unsigned, const float *, unsigned, const float *, unsigned, ResizeGeom, TensorOut); \
        template __global__ void k_to_tensor_resized<NPLANE, kDtypeF32>(const float *, unsigned, const float *, unsigned, const float *, unsigned, ResizeGeom, TensorOut);
J2P_RESIZED_KERNELS(3)
J2P_RESIZED_KERNELS(1)
#undef J2P_RESIZED_KERNELS

// ---------------------------------------------------------------------------
// Filtered tensor output: the box resampled to out_w x out_h — smaller OR larger — with taps from a filter kernel (triangle,
// Keys' cubic), the formula of Pillow and of torch's antialias path.  Every bit is defined (include/jpeg2png_amd.h).
// TAPS: filter_taps below is the header's definition in IEEE double, one operation per line of it; host and device compile
// the same text without contraction, so j2p_debug_filter_taps (host) and k_filter_taps (device) give the same bits.
// k_filter_taps writes both axes' taps into scratch memory — one thread per output index: first[X], count[X] and the f32
// weights at weights + X * stride, stride = ceil(2 * sup) + 2 >= any count (the host's filter_stride) — and
// k_to_tensor_filtered only reads them: the filter is not its template parameter.
// SAMPLING keeps k_to_tensor_resized's shape: a wavefront owns a tile of lanes x slots output columns (column X0 + p * lanes
// + lane in slot p) and `rows` (1..kFilterRows) consecutive output rows; for every source row of those rows' windows, in
// order, it stages the row segment its tile covers in chunks of kResizeChunk columns (16-byte loads aligned down to 4 floats,
// converted ONCE, wave-private LDS, next chunk's loads in flight), every lane walks those taps of its columns that lie in the
// chunk — chunks ascend, so r_j is summed in the defined order — and then every output row of the wavefront whose window
// holds the source row takes acc = acc + fy * r_j: the rows ascend, so acc is summed in the defined order too.
// ONE PASS: r_j is formed again by every wavefront whose rows use source row j, and never stored.  With `rows` output rows
// per wavefront a source row is converted and walked (rows - 1 + 2R) / rows times when shrinking (triangle 1.25x at 4 rows,
// 2x at one; cubic 1.75x and 4x) and about once per wavefront when enlarging, against a two-pass form's once — which would
// pay an f32 intermediate of box_h x out_w x NPLANE floats written and read back (150 MB for 4096x3072 -> 4095x3071).
// LDS: the padded index of the area kernel is kept.  At one tap step neighbouring lanes still read at a stride of box / out
// floats when shrinking (their windows start that far apart), for which the pad was made; when enlarging they read the same
// or the neighbouring word, which the LDS broadcasts.  What is new is that a lane's window is 2R * fs wide instead of
// box / out + 1: neighbouring lanes' windows overlap, and a chunk boundary cuts more windows in two.
// The weights are read from global memory, a lane its own run of floats (a tile's lanes x slots x count floats, read again
// for every source row, stay in L1 / L2).  Tap-major, where the lanes of a wavefront read neighbouring floats at one tap
// step, measured 7 to 11 % SLOWER where the tile was the same: the walk is bound by instructions, and
// a lane's next weight is then a multiplication away instead of one float on.  A tile of 32 columns leaves lanes 32..63
// without taps to walk; giving them the same columns of the next output row (half as many wavefronts, every lane busy) measured
// 1.2 to 1.4 times SLOWER at 224x224: the walk waits for its loads, and more wavefronts hide that better than fuller ones.
// ---------------------------------------------------------------------------
constexpr int kFilterTriangle = 1, kFilterCubic = 2;             // J2P_FILTER_* (checked in j2p_output.hip)
constexpr int kFilterRows = 4;                                   // output rows per wavefront, at most

// w(a), a = |u|
__host__ __device__ inline double filter_weight(int filter, double a)
{
        if(filter == kFilterTriangle) { return a < 1. ? 1. - a : 0.; }
        if(a < 1.) { return ((1.5 * a - 2.5) * a) * a + 1.; }
        if(a < 2.) { return (((a - 5.) * a + 8.) * a - 4.) * -0.5; }
        return 0.;
}

// the taps of output index X of an axis (box, out): *first, *count, and put(t, f_t) for t < min(*count, capacity)
template <typename Put>
__host__ __device__ inline void filter_taps(int filter, unsigned box, unsigned out, unsigned X, unsigned *first, unsigned *count,
                                            unsigned capacity, Put put)
{
        if(out == box) {                                                 // not resized: one tap of weight 1.f
                *first = X;
                *count = 1;
                if(capacity >= 1) { put(0u, 1.f); }
                return;
        }
        const double R = filter == kFilterCubic ? 2. : 1.;
        const double scale = (double)box / (double)out;
        const double fs = scale > 1. ? scale : 1.;
        const double sup = R * fs;
        const double c = ((double)X + 0.5) * scale;
        long long lo = (long long)(c - sup + 0.5), hi = (long long)(c + sup + 0.5);
        if(lo < 0) { lo = 0; }
        if(hi > (long long)box) { hi = (long long)box; }
        double S = 0.;
        for(long long i = lo; i < hi; i++) {
                const double u = (((double)i - c) + 0.5) / fs;
                S = S + filter_weight(filter, __builtin_fabs(u));
        }
        *first = (unsigned)lo;
        *count = (unsigned)(hi - lo);
        for(long long i = lo; i < hi && (unsigned)(i - lo) < capacity; i++) {
                const double u = (((double)i - c) + 0.5) / fs;
                put((unsigned)(i - lo), (float)(filter_weight(filter, __builtin_fabs(u)) / S));
        }
}

struct FilterAxis {
        unsigned box, out, stride;      // stride: weights per output index (>= every count)
        int *first, *count;             // [out]
        float *weights;                 // [out * stride]
};

// blockIdx.y 0: the columns' taps, 1: the rows'
__global__ __launch_bounds__(256) void k_filter_taps(int filter, FilterAxis ax, FilterAxis ay)
{
        const bool rows = blockIdx.y != 0;
        const unsigned box = rows ? ay.box : ax.box, out = rows ? ay.out : ax.out, stride = rows ? ay.stride : ax.stride;
        int *const firsts = rows ? ay.first : ax.first, *const counts = rows ? ay.count : ax.count;
        const unsigned X = blockIdx.x * 256 + threadIdx.x;
        if(X >= out) { return; }
        float *const w = (rows ? ay.weights : ax.weights) + (size_t)X * stride;
        unsigned first = 0, count = 0;
        filter_taps(filter, box, out, X, &first, &count, stride, [&](unsigned t, float f) { w[t] = f; });
        firsts[X] = (int)first;
        counts[X] = (int)(count < stride ? count : stride);              // (never more: see filter_stride)
}

struct FilterGeom {
        unsigned box_x, box_y;
        unsigned out_w, out_h;
        unsigned stride_x, stride_y;    // weights per output column / row
        const int *first_x, *count_x, *first_y, *count_y;
        const float *wx, *wy;
        unsigned lanes, slots;          // the tile: lanes (a power of two, 32 or 64) x slots (1..kResizeSlots) columns
        unsigned rows;                  // consecutive output rows per wavefront: 1..kFilterRows
};

template <int NPLANE, int DTYPE>
__global__ __launch_bounds__(256) void k_to_tensor_filtered(const float *yp, unsigned ys, const float *cbp, unsigned cbs, const float *crp,
                                                            unsigned crs, FilterGeom g, TensorOut o)
{
        static_assert(NPLANE == 1 || NPLANE == 3, "greyscale or RGB");
        constexpr int kRounds = kResizeChunk / 256;
        using E = TensorElement<DTYPE>;
        using Raw = typename E::Raw;
        __shared__ float stage[4][NPLANE][kResizeLds];
        const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
        const unsigned Yb = (blockIdx.y * 4 + (unsigned)wave) * g.rows;   // this wavefront's output rows: [Yb, Yb + nrow)
        if(Yb >= g.out_h) { return; }                                    // (no workgroup barrier in this kernel)
        const unsigned nrow = g.out_h - Yb < g.rows ? g.out_h - Yb : g.rows;
        float (*const lds)[kResizeLds] = stage[wave];
        const unsigned tile = g.lanes * g.slots;
        const unsigned X0 = blockIdx.x * tile;                           // (the grid has no tile beyond out_w)
        const unsigned ncol = g.out_w - X0 < tile ? g.out_w - X0 : tile;
        // the taps of the lane's columns X0 + p * lanes + lane: box columns [fx, fx + nx), weights from wp
        int fx[kResizeSlots], nx[kResizeSlots];
        const float *wp[kResizeSlots];
        bool has[kResizeSlots];
#pragma unroll
        for(int p = 0; p < kResizeSlots; p++) {
                has[p] = (unsigned)p < g.slots && (unsigned)lane < g.lanes && (unsigned)p * g.lanes + (unsigned)lane < ncol;
                const unsigned X = has[p] ? X0 + (unsigned)p * g.lanes + (unsigned)lane : X0;
                fx[p] = g.first_x[X];
                nx[p] = has[p] ? g.count_x[X] : 0;
                wp[p] = g.wx + (size_t)X * g.stride_x;
        }
        // the tile's segment of a source row, in canvas columns: [c_begin, c_last], c_begin a multiple of 4 (first and
        // first + count never decrease from one output index to the next)
        const unsigned Xl = X0 + ncol - 1;
        const int c_last = (int)g.box_x + g.first_x[Xl] + g.count_x[Xl] - 1;
        const int c_begin = ((int)g.box_x + g.first_x[X0]) & ~3;
        // the windows of the wavefront's rows: box rows [fy, fy + ny), the same in every lane; and the source rows of all of
        // them, [j_begin, j_end] (windows never move backwards)
        int fy[kFilterRows], ny[kFilterRows];
#pragma unroll
        for(int q = 0; q < kFilterRows; q++) {
                const bool valid = (unsigned)q < nrow;
                fy[q] = g.first_y[valid ? Yb + (unsigned)q : Yb];
                ny[q] = valid ? g.count_y[Yb + (unsigned)q] : 0;
        }
        const int j_begin = g.first_y[Yb], j_end = g.first_y[Yb + nrow - 1] + g.count_y[Yb + nrow - 1] - 1;
        Raw *const data = static_cast<Raw *>(o.data);

        // the 16-byte loads of chunk c0 of source row j, into registers: issued one chunk ahead of their use
        float4 ld[kRounds][NPLANE];
#pragma unroll
        for(int u = 0; u < kRounds; u++) {
#pragma unroll
                for(int k = 0; k < NPLANE; k++) { ld[u][k] = make_float4(0.f, 0.f, 0.f, 0.f); }
        }
        const auto issue = [&](int j, int c0) {
                const size_t row = (size_t)g.box_y + (size_t)j;
#pragma unroll
                for(int u = 0; u < kRounds; u++) {
                        const int c = c0 + u * 256 + lane * 4;
                        if(c <= c_last) {
                                ld[u][0] = *reinterpret_cast<const float4 *>(yp + row * ys + c);
                                if constexpr(NPLANE == 3) {
                                        ld[u][1] = *reinterpret_cast<const float4 *>(cbp + row * cbs + c);
                                        ld[u][2] = *reinterpret_cast<const float4 *>(crp + row * crs + c);
                                }
                        }
                }
        };

        float acc[kFilterRows][kResizeSlots][NPLANE];
#pragma unroll
        for(int q = 0; q < kFilterRows; q++) {
#pragma unroll
                for(int p = 0; p < kResizeSlots; p++) {
#pragma unroll
                        for(int k = 0; k < NPLANE; k++) { acc[q][p][k] = 0.f; }
                }
        }
        issue(j_begin, c_begin);
        for(int j = j_begin; j <= j_end; j++) {
                // r_j of every column of the lane: the row's chunks, left to right
                float r[kResizeSlots][NPLANE];
#pragma unroll
                for(int p = 0; p < kResizeSlots; p++) {
#pragma unroll
                        for(int k = 0; k < NPLANE; k++) { r[p][k] = 0.f; }
                }
                for(int c0 = c_begin; c0 <= c_last; c0 += kResizeChunk) {
#pragma unroll
                        for(int u = 0; u < kRounds; u++) {
                                const int at = u * 256 + lane * 4;
                                if(c0 + at <= c_last) {
                                        const float yin[4] = {ld[u][0].x, ld[u][0].y, ld[u][0].z, ld[u][0].w};
                                        const float4 cb4 = ld[u][NPLANE == 3 ? 1 : 0], cr4 = ld[u][NPLANE == 3 ? 2 : 0];   // (one plane: not looked at)
                                        const float cbin[4] = {cb4.x, cb4.y, cb4.z, cb4.w}, crin[4] = {cr4.x, cr4.y, cr4.z, cr4.w};
#pragma unroll
                                        for(int q = 0; q < 4; q++) {
                                                const int idx = resize_lds_index(at + q);
                                                clamped_pixel<NPLANE>(yin[q], cbin[q], crin[q], [&](int k, float x) { lds[k][idx] = x; });
                                        }
                                }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        // the next chunk's loads fly while this one's taps are walked
                        if(c0 + kResizeChunk <= c_last) { issue(j, c0 + kResizeChunk); }
                        else if(j < j_end) { issue(j + 1, c_begin); }
                        const int rel0 = c0 - (int)g.box_x;              // the chunk's first column relative to the box (>= -3)
#pragma unroll
                        for(int p = 0; p < kResizeSlots; p++) {
                                if(!has[p]) { continue; }
                                const int i0 = fx[p] > rel0 ? fx[p] : rel0;
                                const int last = fx[p] + nx[p] - 1;
                                const int i1 = last < rel0 + kResizeChunk - 1 ? last : rel0 + kResizeChunk - 1;
                                for(int i = i0; i <= i1; i++) {          // (none of this column's taps in this chunk: i0 > i1)
                                        const float a = wp[p][i - fx[p]];
                                        const int idx = resize_lds_index(i - rel0);
#pragma unroll
                                        for(int k = 0; k < NPLANE; k++) {
                                                const float t = a * lds[k][idx];
                                                r[p][k] = r[p][k] + t;
                                        }
                                }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();                 // the next chunk is staged over this one
                }
                // every output row of the wavefront whose window holds the row takes it with its weight
#pragma unroll
                for(int q = 0; q < kFilterRows; q++) {
                        if(j < fy[q] || j >= fy[q] + ny[q]) { continue; }     // (wavefront-uniform; ny is 0 beyond nrow)
                        const float b = g.wy[(size_t)(Yb + (unsigned)q) * g.stride_y + (unsigned)(j - fy[q])];
#pragma unroll
                        for(int p = 0; p < kResizeSlots; p++) {
#pragma unroll
                                for(int k = 0; k < NPLANE; k++) {
                                        const float t = b * r[p][k];
                                        acc[q][p][k] = acc[q][p][k] + t;
                                }
                        }
                }
        }
#pragma unroll
        for(int q = 0; q < kFilterRows; q++) {
                if((unsigned)q >= nrow) { continue; }
                const long long rowo = (long long)(Yb + (unsigned)q) * o.stride_y;
#pragma unroll
                for(int p = 0; p < kResizeSlots; p++) {
                        if(!has[p]) { continue; }
                        const long long X = (long long)(X0 + (unsigned)p * g.lanes + (unsigned)lane);
#pragma unroll
                        for(int k = 0; k < NPLANE; k++) {
                                float m = acc[q][p][k];
                                m = m > 0.f ? m : 0.f;
                                m = m < 255.f ? m : 255.f;
                                data[(long long)k * o.stride_c + rowo + X * o.stride_x] = (Raw)E::make(m, o.scale[k], o.bias[k]);
                        }
                }
        }
}
#define J2P_FILTERED_KERNELS(NPLANE)                                                                                                          \
        template __global__ void k_to_tensor_filtered<NPLANE, kDtypeU8>(const float *, unsigned, const float *, unsigned, const float *, unsigned, FilterGeom, TensorOut);   \
        template __global__ void k_to_tensor_filtered<NPLANE, kDtypeF16>(const float *, unsigned, const float *, unsigned, const float *, unsigned, FilterGeom, TensorOut);  \
        template __global__ void k_to_tensor_filtered<NPLANE, kDtypeBF16>(const float *, unsigned, const float *, unsigned, const float *, unsigned, FilterGeom, TensorOut); \
        template __global__ void k_to_tensor_filtered<NPLANE, kDtypeF32>(const float *, unsigned, const float *, unsigned, const float *, unsigned, FilterGeom, TensorOut);
J2P_FILTERED_KERNELS(3)
J2P_FILTERED_KERNELS(1)
#undef J2P_FILTERED_KERNELS

// ---------------------------------------------------------------------------
// JPEG output: a solved plane straight to quantised coefficients — dct8x8s (ooura/dct.c:98-130) of every 8x8 block,
// each coefficient divided by its output quantisation step (IEEE f32 quotient: `/` under
// -fhip-fp32-correctly-rounded-divide-sqrt, never a reciprocal multiply), rounded to nearest even, clamped to
// [-1023, 1023] (what libjpeg's Huffman coder takes: AC magnitudes of at most 10 bits, DC differences of at most 11).
// No +128: JPEG's level shift and the luma fix-up of jpeg2png.c:156-159 cancel.
// out: block-major int16 [blocks][64], natural order — the JBLOCK rows of libjpeg.
// Mapping of k_dct_blocks: one wavefront = 8 horizontally adjacent blocks, lane >> 3 the block, lane & 7 the row; a
// lane stores its 8 coefficients as one 16-byte vector (the wavefront: 1 KB contiguous).
// ---------------------------------------------------------------------------
struct QuantSteps {
        float q[64];        // natural order
};

// the tail: a lane holds row `lane & 7` of block `lane >> 3` of its wavefront's 8 blocks in v[];
// dct8x8s, quotient, rounding, clamp, and the row's 8 coefficients as one 16-byte store into `block` (ok lanes only)
__device__ __forceinline__ void quantise_store(float (&v)[8], float *scratch, const float *qs, int lane, bool ok, int16_t *block)
{
        const int rr = lane & 7;
        transpose8(v, scratch, lane);
        fdct8(v);
        transpose8(v, scratch, lane);
        fdct8(v);
        unsigned packed[4];
#pragma unroll
        for(int u = 0; u < 8; u += 2) {
                unsigned half[2];
#pragma unroll
                for(int k = 0; k < 2; k++) {
                        float t = rintf(v[u + k] / qs[rr * 8 + u + k]);
                        t = t > 1023.f ? 1023.f : (t < -1023.f ? -1023.f : t);
                        half[k] = (unsigned)(int)t & 0xffffu;
                }
                packed[u / 2] = half[0] | (half[1] << 16);
        }
        if(ok) { *reinterpret_cast<uint4 *>(block + rr * 8) = make_uint4(packed[0], packed[1], packed[2], packed[3]); }
}

// ---------------------------------------------------------------------------
// One kernel for every output sampling (4:4:4, 4:2:2, 4:2:0, 4:4:0): output sample (X, Y) of the block grid is the mean
// the projection constrains (compute.c:351-359) — a float accumulator that starts at 0.f takes the SY * SX canvas values
// at rows Y * SY + j, columns X * SX + i in raster order (j outer, i inner), one addition each, and is divided by
// (float)(SX * SY) — and the 8x8 blocks of those samples go through the transform, quotient, rounding and clamp above.
// <1, 1> gives the coefficients of the plane itself: (0.f + x) / 1.f differs from x only for x = -0.f, which becomes
// +0.f; another sign on a zero input can only change the sign of a zero somewhere in the two fdct8 passes, and every
// such zero ends as the integer 0 after rintf and the conversion to int.
// plane: first row = the first canvas row of the block_rows output block rows; stride x rows: what the canvas holds from
// there on.  out: block-major int16 [block_rows * blocks_w][64].  A row index beyond the canvas's last row reads the
// last row, a column beyond the last column the last column: only the last block row / column of a grid that overhangs
// the canvas (every block STARTS inside it, which the host checks; never for <1, 1>, where canvas, band cuts and
// blocks_w * 8 are all multiples of 8).  A lane loads SY rows of 8 * SX consecutive floats as float4 (a block starts at
// a multiple of 8 * SX floats and the stride is a multiple of 8: aligned), 8 lanes 256 * SX contiguous bytes of a canvas
// row; only lanes whose footprint crosses the canvas's edge take the clamped scalar loads.
// ---------------------------------------------------------------------------
template <int SX, int SY>
__global__ __launch_bounds__(256) void k_quantise_blocks(const float *plane, unsigned stride, unsigned rows, unsigned blocks_w,
                                                         unsigned block_rows, QuantSteps steps, int16_t *out)
{
        static_assert((SX == 1 || SX == 2) && (SY == 1 || SY == 2), "sampling factors 1 and 2");
        __shared__ __attribute__((aligned(16))) float tp[4 * kTpWave];
        __shared__ float qs[64];
        if(threadIdx.x < 64) { qs[threadIdx.x] = steps.q[threadIdx.x]; }
        __syncthreads();
        const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
        const unsigned groups_x = (blocks_w + 7) / 8;
        const unsigned grp = blockIdx.x * 4 + wave;
        if(grp >= groups_x * block_rows) { return; }                    // whole wavefronts only: no barrier follows
        const unsigned by = grp / groups_x, bx = (grp % groups_x) * 8 + (unsigned)(lane >> 3);
        const int rr = lane & 7;
        const bool ok = bx < blocks_w;
        const unsigned x0 = bx * (8 * SX), y0 = (by * 8 + (unsigned)rr) * SY;
        float v[8];
#pragma unroll
        for(int u = 0; u < 8; u++) { v[u] = 0.f; }
        const bool inside = SX * SY == 1 || (x0 + 8 * SX <= stride && y0 + SY <= rows);         // (<1, 1>: nothing can overhang)
        if(ok && inside) {
#pragma unroll
                for(int j = 0; j < SY; j++) {
                        const float4 *src = reinterpret_cast<const float4 *>(plane + (size_t)(y0 + j) * stride + x0);
                        float f[8 * SX];
#pragma unroll
                        for(int k = 0; k < 2 * SX; k++) {
                                const float4 a = src[k];
                                f[4 * k] = a.x; f[4 * k + 1] = a.y; f[4 * k + 2] = a.z; f[4 * k + 3] = a.w;
                        }
#pragma unroll
                        for(int u = 0; u < 8; u++) {
#pragma unroll
                                for(int i = 0; i < SX; i++) { v[u] = v[u] + f[u * SX + i]; }
                        }
                }
        } else if(ok) {
                // the footprint crosses the canvas's last column or row: replicate them
#pragma unroll
                for(int j = 0; j < SY; j++) {
                        const unsigned y = y0 + j < rows ? y0 + j : rows - 1;
                        const float *src = plane + (size_t)y * stride;
#pragma unroll
                        for(int u = 0; u < 8; u++) {
#pragma unroll
                                for(int i = 0; i < SX; i++) {
                                        const unsigned x = x0 + u * SX + i;
                                        v[u] = v[u] + src[x < stride ? x : stride - 1];
                                }
                        }
                }
        }
#pragma unroll
        for(int u = 0; u < 8; u++) { v[u] = v[u] / (float)(SX * SY); }
        quantise_store(v, tp + wave * kTpWave, qs, lane, ok, out + ((size_t)by * blocks_w + bx) * 64);
}
// (explicit instantiations, as for k_to_samples)
template __global__ void k_quantise_blocks<1, 1>(const float *, unsigned, unsigned, unsigned, unsigned, QuantSteps, int16_t *);
template __global__ void k_quantise_blocks<2, 2>(const float *, unsigned, unsigned, unsigned, unsigned, QuantSteps, int16_t *);
template __global__ void k_quantise_blocks<2, 1>(const float *, unsigned, unsigned, unsigned, unsigned, QuantSteps, int16_t *);
template __global__ void k_quantise_blocks<1, 2>(const float *, unsigned, unsigned, unsigned, unsigned, QuantSteps, int16_t *);

// ---------------------------------------------------------------------------
// Several filtered outputs in one call (j2p_planes_to_tensors_resampled): one launch for the taps of every axis of every
// output, one sampling launch per dtype.  Kernels of their own BESIDE k_filter_taps and k_to_tensor_filtered, at the end of the
// code object, and the tile's text a second time: with one device function under both sampling kernels the single call's
// kernel came out of the compiler with another schedule and register count, and its time moved by -5 to +6 % depending on the
// shape, where two builds of one source differ by 0.5 % at most.  filtered_tile IS
// k_to_tensor_filtered's body with the tile column and the row group as arguments — the same staging, the same ascending
// chunk and row order, the same bits; a change to one belongs in the other (tests/test_outputs_gpu.py compares their bits).
// ---------------------------------------------------------------------------
// the taps of index X of one axis into its arrays
__device__ __forceinline__ void filter_axis_taps(int filter, const FilterAxis &a, unsigned X)
{
        float *const w = a.weights + (size_t)X * a.stride;
        unsigned first = 0, count = 0;
        filter_taps(filter, a.box, a.out, X, &first, &count, a.stride, [&](unsigned t, float f) { w[t] = f; });
        a.first[X] = (int)first;
        a.count[X] = (int)(count < a.stride ? count : a.stride);         // (never more: see filter_stride)
}


// Several outputs in one launch (j2p_planes_to_tensors_resampled): the launch's workgroups are those of the outputs' own
// launches one after the other, end[i] the number of workgroups of outputs 0..i.  The output of workgroup `wg` and the
// workgroup's index among that output's own: host and device compile this text (j2p_debug_outputs_workgroups).
constexpr int kMaxOutputs = 16;                                  // J2P_MAX_OUTPUTS (checked in j2p_output.hip)
__host__ __device__ inline unsigned output_of_workgroup(const unsigned *end, unsigned n, unsigned wg, unsigned *local)
{
        unsigned i = 0;
        while(i + 1 < n && wg >= end[i]) { i++; }
        *local = wg - (i ? end[i - 1] : 0);
        return i;
}

// the taps of every axis of every output of a call in one launch: 2 * outputs axes, each with its filter and the workgroups
// (of 256 indices) it needs — no workgroup without work
struct FilterAxes {
        unsigned n;                                      // axes: at most 2 * kMaxOutputs
        unsigned end[2 * kMaxOutputs];
        int filter[2 * kMaxOutputs];
        FilterAxis axis[2 * kMaxOutputs];
};
__global__ __launch_bounds__(256) void k_filter_taps_outputs(FilterAxes axes)
{
        unsigned local;
        const unsigned i = output_of_workgroup(axes.end, axes.n, blockIdx.x, &local);
        const FilterAxis &a = axes.axis[i];
        const unsigned X = local * 256 + threadIdx.x;
        if(X >= a.out) { return; }
        filter_axis_taps(axes.filter[i], a, X);
}

// one workgroup's work: tile column bx, row group by (4 wavefronts, one above the other) of the output g, o
template <int NPLANE, int DTYPE>
__device__ __forceinline__ void filtered_tile(const float *yp, unsigned ys, const float *cbp, unsigned cbs, const float *crp, unsigned crs,
                                              const FilterGeom &g, const TensorOut &o, unsigned bx, unsigned by)
{
        static_assert(NPLANE == 1 || NPLANE == 3, "greyscale or RGB");
        constexpr int kRounds = kResizeChunk / 256;
        using E = TensorElement<DTYPE>;
        using Raw = typename E::Raw;
        __shared__ float stage[4][NPLANE][kResizeLds];
        const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
        const unsigned Yb = (by * 4 + (unsigned)wave) * g.rows;           // this wavefront's output rows: [Yb, Yb + nrow)
        if(Yb >= g.out_h) { return; }                                    // (no workgroup barrier in this kernel)
        const unsigned nrow = g.out_h - Yb < g.rows ? g.out_h - Yb : g.rows;
        float (*const lds)[kResizeLds] = stage[wave];
        const unsigned tile = g.lanes * g.slots;
        const unsigned X0 = bx * tile;                                   // (the grid has no tile beyond out_w)
        const unsigned ncol = g.out_w - X0 < tile ? g.out_w - X0 : tile;
        // the taps of the lane's columns X0 + p * lanes + lane: box columns [fx, fx + nx), weights from wp
        int fx[kResizeSlots], nx[kResizeSlots];
        const float *wp[kResizeSlots];
        bool has[kResizeSlots];
#pragma unroll
        for(int p = 0; p < kResizeSlots; p++) {
                has[p] = (unsigned)p < g.slots && (unsigned)lane < g.lanes && (unsigned)p * g.lanes + (unsigned)lane < ncol;
                const unsigned X = has[p] ? X0 + (unsigned)p * g.lanes + (unsigned)lane : X0;
                fx[p] = g.first_x[X];
                nx[p] = has[p] ? g.count_x[X] : 0;
                wp[p] = g.wx + (size_t)X * g.stride_x;
        }
        // the tile's segment of a source row, in canvas columns: [c_begin, c_last], c_begin a multiple of 4 (first and
        // first + count never decrease from one output index to the next)
        const unsigned Xl = X0 + ncol - 1;
        const int c_last = (int)g.box_x + g.first_x[Xl] + g.count_x[Xl] - 1;
        const int c_begin = ((int)g.box_x + g.first_x[X0]) & ~3;
        // the windows of the wavefront's rows: box rows [fy, fy + ny), the same in every lane; and the source rows of all of
        // them, [j_begin, j_end] (windows never move backwards)
        int fy[kFilterRows], ny[kFilterRows];
#pragma unroll
        for(int q = 0; q < kFilterRows; q++) {
                const bool valid = (unsigned)q < nrow;
                fy[q] = g.first_y[valid ? Yb + (unsigned)q : Yb];
                ny[q] = valid ? g.count_y[Yb + (unsigned)q] : 0;
        }
        const int j_begin = g.first_y[Yb], j_end = g.first_y[Yb + nrow - 1] + g.count_y[Yb + nrow - 1] - 1;
        Raw *const data = static_cast<Raw *>(o.data);

        // the 16-byte loads of chunk c0 of source row j, into registers: issued one chunk ahead of their use
        float4 ld[kRounds][NPLANE];
#pragma unroll
        for(int u = 0; u < kRounds; u++) {
#pragma unroll
                for(int k = 0; k < NPLANE; k++) { ld[u][k] = make_float4(0.f, 0.f, 0.f, 0.f); }
        }
        const auto issue = [&](int j, int c0) {
                const size_t row = (size_t)g.box_y + (size_t)j;
#pragma unroll
                for(int u = 0; u < kRounds; u++) {
                        const int c = c0 + u * 256 + lane * 4;
                        if(c <= c_last) {
                                ld[u][0] = *reinterpret_cast<const float4 *>(yp + row * ys + c);
                                if constexpr(NPLANE == 3) {
                                        ld[u][1] = *reinterpret_cast<const float4 *>(cbp + row * cbs + c);
                                        ld[u][2] = *reinterpret_cast<const float4 *>(crp + row * crs + c);
                                }
                        }
                }
        };

        float acc[kFilterRows][kResizeSlots][NPLANE];
#pragma unroll
        for(int q = 0; q < kFilterRows; q++) {
#pragma unroll
                for(int p = 0; p < kResizeSlots; p++) {
#pragma unroll
                        for(int k = 0; k < NPLANE; k++) { acc[q][p][k] = 0.f; }
                }
        }
        issue(j_begin, c_begin);
        for(int j = j_begin; j <= j_end; j++) {
                // r_j of every column of the lane: the row's chunks, left to right
                float r[kResizeSlots][NPLANE];
#pragma unroll
                for(int p = 0; p < kResizeSlots; p++) {
#pragma unroll
                        for(int k = 0; k < NPLANE; k++) { r[p][k] = 0.f; }
                }
                for(int c0 = c_begin; c0 <= c_last; c0 += kResizeChunk) {
#pragma unroll
                        for(int u = 0; u < kRounds; u++) {
                                const int at = u * 256 + lane * 4;
                                if(c0 + at <= c_last) {
                                        const float yin[4] = {ld[u][0].x, ld[u][0].y, ld[u][0].z, ld[u][0].w};
                                        const float4 cb4 = ld[u][NPLANE == 3 ? 1 : 0], cr4 = ld[u][NPLANE == 3 ? 2 : 0];   // (one plane: not looked at)
                                        const float cbin[4] = {cb4.x, cb4.y, cb4.z, cb4.w}, crin[4] = {cr4.x, cr4.y, cr4.z, cr4.w};
#pragma unroll
                                        for(int q = 0; q < 4; q++) {
                                                const int idx = resize_lds_index(at + q);
                                                clamped_pixel<NPLANE>(yin[q], cbin[q], crin[q], [&](int k, float x) { lds[k][idx] = x; });
                                        }
                                }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        // the next chunk's loads fly while this one's taps are walked
                        if(c0 + kResizeChunk <= c_last) { issue(j, c0 + kResizeChunk); }
                        else if(j < j_end) { issue(j + 1, c_begin); }
                        const int rel0 = c0 - (int)g.box_x;              // the chunk's first column relative to the box (>= -3)
#pragma unroll
                        for(int p = 0; p < kResizeSlots; p++) {
                                if(!has[p]) { continue; }
                                const int i0 = fx[p] > rel0 ? fx[p] : rel0;
                                const int last = fx[p] + nx[p] - 1;
                                const int i1 = last < rel0 + kResizeChunk - 1 ? last : rel0 + kResizeChunk - 1;
                                for(int i = i0; i <= i1; i++) {          // (none of this column's taps in this chunk: i0 > i1)
                                        const float a = wp[p][i - fx[p]];
                                        const int idx = resize_lds_index(i - rel0);
#pragma unroll
                                        for(int k = 0; k < NPLANE; k++) {
                                                const float t = a * lds[k][idx];
                                                r[p][k] = r[p][k] + t;
                                        }
                                }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();                 // the next chunk is staged over this one
                }
                // every output row of the wavefront whose window holds the row takes it with its weight
#pragma unroll
                for(int q = 0; q < kFilterRows; q++) {
                        if(j < fy[q] || j >= fy[q] + ny[q]) { continue; }     // (wavefront-uniform; ny is 0 beyond nrow)
                        const float b = g.wy[(size_t)(Yb + (unsigned)q) * g.stride_y + (unsigned)(j - fy[q])];
#pragma unroll
                        for(int p = 0; p < kResizeSlots; p++) {
#pragma unroll
                                for(int k = 0; k < NPLANE; k++) {
                                        const float t = b * r[p][k];
                                        acc[q][p][k] = acc[q][p][k] + t;
                                }
                        }
                }
        }
#pragma unroll
        for(int q = 0; q < kFilterRows; q++) {
                if((unsigned)q >= nrow) { continue; }
                const long long rowo = (long long)(Yb + (unsigned)q) * o.stride_y;
#pragma unroll
                for(int p = 0; p < kResizeSlots; p++) {
                        if(!has[p]) { continue; }
                        const long long X = (long long)(X0 + (unsigned)p * g.lanes + (unsigned)lane);
#pragma unroll
                        for(int k = 0; k < NPLANE; k++) {
                                float m = acc[q][p][k];
                                m = m > 0.f ? m : 0.f;
                                m = m < 255.f ? m : 255.f;
                                data[(long long)k * o.stride_c + rowo + X * o.stride_x] = (Raw)E::make(m, o.scale[k], o.bias[k]);
                        }
                }
        }
}
// Several outputs of one dtype in one launch: a grid of exactly the workgroups the outputs' own launches have, flattened.  A
// workgroup finds its output in the prefix table and from its index among that output's own the tile column (fastest, as
// blockIdx.x is) and the row group; then it does what k_to_tensor_filtered's workgroup of that place does — same staging, same
// ascending chunk and row order, same bits.  The views of one call differ in size by 5x and more: a grid sized for the largest
// would mostly exit early, this one launches no workgroup without work.  Geometry and destinations are kernel arguments (16 of
// each, 2.4 KB of the 4 KB there are): nothing is copied to the device for them, and the workgroup's own pair is read with
// scalar loads at a uniform index.
struct FilterOutputs {
        unsigned n;
        unsigned end[kMaxOutputs];                       // workgroups of outputs 0..i
        unsigned columns[kMaxOutputs];                   // tile columns of output i: its own grid's x dimension
        FilterGeom g[kMaxOutputs];
        TensorOut o[kMaxOutputs];
};
static_assert(sizeof(FilterOutputs) + 6 * 8 <= 4096, "kernel arguments: 4 KB");

template <int NPLANE, int DTYPE>
__global__ __launch_bounds__(256) void k_to_tensors_filtered(const float *yp, unsigned ys, const float *cbp, unsigned cbs, const float *crp,
                                                             unsigned crs, FilterOutputs a)
{
        unsigned local;
        const unsigned i = output_of_workgroup(a.end, a.n, blockIdx.x, &local);
        const unsigned columns = a.columns[i], by = local / columns;
        filtered_tile<NPLANE, DTYPE>(yp, ys, cbp, cbs, crp, crs, a.g[i], a.o[i], local - by * columns, by);
}
#define J2P_FILTERED_OUTPUTS_KERNELS(NPLANE)                                                                                                  \
        template __global__ void k_to_tensors_filtered<NPLANE, kDtypeU8>(const float *, unsigned, const float *, unsigned, const float *, unsigned, FilterOutputs);   \
        template __global__ void k_to_tensors_filtered<NPLANE, kDtypeF16>(const float *, unsigned, const float *, unsigned, const float *, unsigned, FilterOutputs);  \
        template __global__ void k_to_tensors_filtered<NPLANE, kDtypeBF16>(const float *, unsigned, const float *, unsigned, const float *, unsigned, FilterOutputs); \
        template __global__ void k_to_tensors_filtered<NPLANE, kDtypeF32>(const float *, unsigned, const float *, unsigned, const float *, unsigned, FilterOutputs);
J2P_FILTERED_OUTPUTS_KERNELS(3)
J2P_FILTERED_OUTPUTS_KERNELS(1)
#undef J2P_FILTERED_OUTPUTS_KERNELS

// ---------------------------------------------------------------------------
// Upright planes: the EXIF orientation (2..8) applied to a solver's current iterate as a pure permutation, replication
// included (include/jpeg2png_amd.h: j2p_solver_set_orientation states the map).  U[y][x] = I[sy][sx] for every (x, y) of the
// upright canvas UW x UH; beyond the upright image uw x uh the destination coordinate is clamped BEFORE the map, so the
// canvas's last columns and rows replicate the image's and every load stays inside the source image.  No arithmetic touches
// a value: every output form on U gives the bits it gives on a canvas that held U.
// With (u, v) = (x, y), or (y, x) for the transposing orientations 5..8: sx = flip_x ? w - 1 - u : u, sy = flip_y ? h - 1 - v : v.
// Up to three planes per launch (blockIdx.z), named members picked with compares: an array among the kernel arguments,
// indexed by a register or merely passed on by reference, is copied into private memory.
// ---------------------------------------------------------------------------
struct UprightGeom {
        unsigned w, h;                  // the source image
        unsigned uw, uh;                // the upright image: w x h, or h x w when transposing
        unsigned UW, UH;                // the upright canvas (the destination's stride and rows)
        unsigned src_stride;            // the solver's canvas width
        unsigned flip_x, flip_y;
};
struct UprightPlanes {
        const float *src0, *src1, *src2;
        float *dst0, *dst1, *dst2;
};

// Orientations 2..4: rows stay rows.  A workgroup copies 4 destination rows x 256 columns, a lane one column of each row: a
// wavefront's loads and stores are 256 consecutive bytes either way (a reversed row is read backwards, lane by lane, from
// the same lines).
__global__ __launch_bounds__(256) void k_upright_rows(UprightPlanes p, UprightGeom g)
{
        const float *src = blockIdx.z == 0 ? p.src0 : (blockIdx.z == 1 ? p.src1 : p.src2);
        float *dst = blockIdx.z == 0 ? p.dst0 : (blockIdx.z == 1 ? p.dst1 : p.dst2);
        const unsigned x = blockIdx.x * 256 + threadIdx.x;
        if(x >= g.UW) { return; }
        const unsigned cx = x < g.uw ? x : g.uw - 1;
        const unsigned sx = g.flip_x ? g.w - 1 - cx : cx;
        float v[4];
#pragma unroll
        for(unsigned k = 0; k < 4; k++) {
                const unsigned y = blockIdx.y * 4 + k;
                const unsigned cy = y < g.uh ? y : g.uh - 1;
                const unsigned sy = g.flip_y ? g.h - 1 - cy : cy;
                v[k] = src[(size_t)sy * g.src_stride + sx];
        }
#pragma unroll
        for(unsigned k = 0; k < 4; k++) {
                const unsigned y = blockIdx.y * 4 + k;
                if(y < g.UH) { dst[(size_t)y * g.UW + x] = v[k]; }
        }
}

// Orientations 5..8: a destination tile of kUprightTile x kUprightTile goes through LDS.  Loading, wavefront r of 4 takes the
// tile's destination columns i = r, r + 4, ...: those are source ROWS, and its lanes j run along the source row (the
// destination's y), so a load instruction reads 256 consecutive bytes.  Storing, a wavefront takes destination rows j and its
// lanes i run along x: 256 consecutive bytes again.  The tile is tile[i][j] with a pitch of kUprightTile + 1 floats: the
// row-wise ds_write_b32 of the load phase puts a half-wavefront's 32 lanes on 32 consecutive banks, and the column-wise
// ds_read_b32 of the store phase reads lane i at dword i * 65 + j, bank (i + j) % 32 — distinct over the 32 lanes that
// can conflict.  16.25 KiB per workgroup.
constexpr int kUprightTile = 64;
__global__ __launch_bounds__(256) void k_upright_transpose(UprightPlanes p, UprightGeom g)
{
        __shared__ float tile[kUprightTile][kUprightTile + 1];
        const float *src = blockIdx.z == 0 ? p.src0 : (blockIdx.z == 1 ? p.src1 : p.src2);
        float *dst = blockIdx.z == 0 ? p.dst0 : (blockIdx.z == 1 ? p.dst1 : p.dst2);
        const unsigned lane = threadIdx.x % 64, wave = threadIdx.x / 64;
        const unsigned x0 = blockIdx.x * kUprightTile, y0 = blockIdx.y * kUprightTile;
        {
                const unsigned y = y0 + lane;
                const unsigned cy = y < g.uh ? y : g.uh - 1;
                const unsigned sx = g.flip_x ? g.w - 1 - cy : cy;
#pragma unroll 4
                for(unsigned i = wave; i < (unsigned)kUprightTile; i += 4) {
                        const unsigned x = x0 + i;
                        const unsigned cx = x < g.uw ? x : g.uw - 1;
                        const unsigned sy = g.flip_y ? g.h - 1 - cx : cx;
                        tile[i][lane] = src[(size_t)sy * g.src_stride + sx];
                }
        }
        __syncthreads();
        const unsigned x = x0 + lane;
        if(x >= g.UW) { return; }
#pragma unroll 4
        for(unsigned j = wave; j < (unsigned)kUprightTile; j += 4) {
                const unsigned y = y0 + j;
                if(y < g.UH) { dst[(size_t)y * g.UW + x] = tile[lane][j]; }
        }
}

}  // namespace j2p
