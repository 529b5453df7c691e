// jpeg2png_amd — the 8-point DCT passes, the 8x8 lane transpose and the load of a block row's 8-bit samples: the device code
// that the solver's kernels (j2p_kernels.hip.h), the output stage's (j2p_output_kernels.hip.h) and the table estimator's
// (j2p_estimate_kernels.hip.h) share.  Nothing else is shared between the device translation units.  Bit-exactness rules:
// see j2p_kernels.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace j2p {

// ---------------------------------------------------------------------------
// 8-point orthonormal DCT-II / DCT-III, one lane owns the whole 8-vector.
// ---------------------------------------------------------------------------
// sqrt(2/8)*cos(k*pi/16), sqrt(2/8)*sin(k*pi/16), and cos(pi/4) — the values of
// ooura/dct.c:24-31, kept as double so that products promote like the reference.
constexpr double K1c = 0.49039264020161522456, K1s = 0.09754516100806413392;
constexpr double K2c = 0.46193976625564337806, K2s = 0.19134171618254488586;
constexpr double K3c = 0.41573480615127261854, K3s = 0.27778511650980111237;
constexpr double K4 = 0.35355339059327376220, KH = 0.70710678118654752440;

__device__ __forceinline__ float mix_add(double ka, float a, double kb, float b)
{
        return (float)(ka * (double)a + kb * (double)b);
}
__device__ __forceinline__ float mix_sub(double ka, float a, double kb, float b)
{
        return (float)(ka * (double)a - kb * (double)b);
}
__device__ __forceinline__ float scale(double k, float a) { return (float)(k * (double)a); }

// one pass of dct8x8s (ooura/dct.c:103-130)
__device__ __forceinline__ void fdct8(float (&v)[8])
{
        float e0 = v[0] + v[7], o0 = v[0] - v[7];
        float e1 = v[2] + v[5], o1 = v[2] - v[5];
        float e2 = v[4] + v[3], o2 = v[4] - v[3];
        float e3 = v[6] + v[1], o3 = v[6] - v[1];
        float p = e0 + e2, q = e1 + e3;
        v[0] = scale(K4, p + q);
        v[4] = scale(K4, p - q);
        p = e0 - e2;
        q = e1 - e3;
        v[2] = mix_sub(K2c, p, K2s, q);
        v[6] = mix_add(K2c, q, K2s, p);
        float r = scale(KH, o1 - o3);
        float t = scale(KH, o1 + o3);
        float u3 = t - o2;
        float u1 = t + o2;
        float w3 = o0 - r;
        float w1 = o0 + r;
        v[1] = mix_sub(K1c, w1, K1s, u1);
        v[7] = mix_add(K1c, u1, K1s, w1);
        v[3] = mix_sub(K3c, w3, K3s, u3);
        v[5] = mix_add(K3c, u3, K3s, w3);
}

// one pass of idct8x8s (ooura/dct.c:39-66)
__device__ __forceinline__ void idct8(float (&v)[8])
{
        float a1 = mix_add(K1c, v[1], K1s, v[7]);
        float b1 = mix_sub(K1c, v[7], K1s, v[1]);
        float a3 = mix_add(K3c, v[3], K3s, v[5]);
        float b3 = mix_sub(K3c, v[5], K3s, v[3]);
        float dr = a1 - a3;
        float di = b1 + b3;
        a1 = a1 + a3;
        b3 = b3 - b1;
        b1 = scale(KH, dr + di);
        a3 = scale(KH, dr - di);
        float cr = mix_add(K2c, v[2], K2s, v[6]);
        float ci = mix_sub(K2c, v[6], K2s, v[2]);
        float s0 = scale(K4, v[0] + v[4]);
        float d0 = scale(K4, v[0] - v[4]);
        float m2r = s0 - cr;
        float m2i = d0 - ci;
        s0 = s0 + cr;
        d0 = d0 + ci;
        v[0] = s0 + a1;
        v[7] = s0 - a1;
        v[2] = d0 + b1;
        v[5] = d0 - b1;
        v[4] = m2r - b3;
        v[3] = m2r + b3;
        v[6] = m2i - a3;
        v[1] = m2i + a3;
}

// ---------------------------------------------------------------------------
// 8x8 transpose inside each group of 8 lanes through wave-private LDS.
// Lane (b = lane>>3, j = lane&7) owns 8 values v[0..7] of line j of block b and
// receives element j of every line: out[i] = v_of_lane(b,i)[j].
// Layout b*104 + line*12 + elem: the two 16-byte stores of a lane group hit 32
// distinct banks (12*j mod 32 covers all 4-bank slots), and the dword reads of a
// 32-lane half hit 32 distinct banks (104 mod 32 = 8).
// ---------------------------------------------------------------------------
constexpr int kTpLine = 12, kTpBlock = 104, kTpWave = 8 * kTpBlock;  // floats

__device__ __forceinline__ void transpose8(float (&v)[8], float *scratch, int lane)
{
        const int b = lane >> 3, j = lane & 7;
        float4 *dst = reinterpret_cast<float4 *>(scratch + b * kTpBlock + j * kTpLine);
        dst[0] = make_float4(v[0], v[1], v[2], v[3]);
        dst[1] = make_float4(v[4], v[5], v[6], v[7]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const float *src = scratch + b * kTpBlock + j;
#pragma unroll
        for(int i = 0; i < 8; i++) { v[i] = src[i * kTpLine]; }
        __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------
// One lane's 8 samples of a block row, stride_x bytes apart from src — the load of sample input (k_samples_to_coefficients)
// and of the histogram of j2p_estimate_kernels.hip.h.  `wide` (stride_x == 1 and src a multiple of 8: the host says so): one
// 8-byte load, 8 lanes 64 contiguous bytes of a row; otherwise 8 byte loads.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void load_samples8(const uint8_t *src, ptrdiff_t stride_x, int wide, unsigned (&s)[8])
{
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        if(wide) {
                const v2u r = *reinterpret_cast<const v2u *>(src);
#pragma unroll
                for(int u = 0; u < 4; u++) {
                        s[u] = (r.x >> (8 * u)) & 0xffu;
                        s[4 + u] = (r.y >> (8 * u)) & 0xffu;
                }
        } else {
#pragma unroll
                for(int u = 0; u < 8; u++) { s[u] = src[(ptrdiff_t)u * stride_x]; }
        }
}

}  // namespace j2p
