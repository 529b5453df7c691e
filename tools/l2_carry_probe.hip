// Does an XCD's L2 keep its lines across a dependent kernel boundary — and can a per-dispatch counter run see it?
// Stand-alone probe (hipcc --offload-arch=gfx950 -O2 tools/l2_carry_probe.hip -o l2_carry_probe).
//
// Workgroup b runs on XCD b % 8.  k_first gives XCD q the q-th contiguous eighth (2 MiB, half an L2) of a 16 MiB buffer.
// k_again_same reads the buffer again with the same map: every line it wants is where its XCD's L2 left it.
// k_again_shifted reads it with the eighths moved on by one XCD: the same bytes, but every line sits in a neighbour's L2.
// k_evict reads 64 MiB of something else in between, so that every round starts alike.
//   plain run:            HIP-event time of the two second kernels (median of the rounds)
//   under a counter run:  FETCH_SIZE of the two second kernels; if k_again_same fetches the whole buffer there although it
//                         is the faster one in the plain run, the counter run itself empties the L2s between dispatches
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define TRY(x) do { hipError_t e_ = (x); if(e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while(0)

__device__ __forceinline__ void touch(const float4 *src, float *out, unsigned chunk, unsigned shift)
{
        const unsigned b = blockIdx.x, per = gridDim.x >> 3;                  // (gridDim.x is a multiple of 8)
        const unsigned q = ((b & 7) + shift) & 7, j = b >> 3;
        const float4 *p = src + (size_t)(q * per + j) * chunk;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for(unsigned i = threadIdx.x; i < chunk; i += 256) {
                const float4 v = p[i];
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        out[(size_t)b * 256 + threadIdx.x] = (acc.x + acc.y) + (acc.z + acc.w);
}
__global__ __launch_bounds__(256) void k_first(const float4 *src, float *out, unsigned chunk) { touch(src, out, chunk, 0); }
__global__ __launch_bounds__(256) void k_again_same(const float4 *src, float *out, unsigned chunk) { touch(src, out, chunk, 0); }
__global__ __launch_bounds__(256) void k_again_shifted(const float4 *src, float *out, unsigned chunk) { touch(src, out, chunk, 1); }
__global__ __launch_bounds__(256) void k_evict(const float4 *src, float *out, unsigned chunk) { touch(src, out, chunk, 0); }

int main(int argc, char **argv)
{
        const int rounds = argc > 1 ? atoi(argv[1]) : 50;
        const unsigned nwg = 2048, chunk = 512;                               // 2048 x 512 float4 = 16 MiB
        const size_t bytes = (size_t)nwg * chunk * sizeof(float4), big = 4 * bytes;
        float4 *buf = nullptr, *other = nullptr;
        float *out = nullptr;
        TRY(hipMalloc(&buf, bytes));
        TRY(hipMalloc(&other, big));
        TRY(hipMalloc(&out, (size_t)nwg * 256 * sizeof(float)));
        TRY(hipMemset(buf, 0, bytes));
        TRY(hipMemset(other, 0, big));
        hipEvent_t e0, e1;
        TRY(hipEventCreate(&e0));
        TRY(hipEventCreate(&e1));
        std::vector<float> same, shifted;
        for(int r = 0; r < rounds; r++) {
                for(int form = 0; form < 2; form++) {
                        hipLaunchKernelGGL(k_evict, dim3(nwg), dim3(256), 0, 0, other, out, 4 * chunk);
                        hipLaunchKernelGGL(k_first, dim3(nwg), dim3(256), 0, 0, buf, out, chunk);
                        TRY(hipEventRecord(e0, 0));
                        if(form == 0) { hipLaunchKernelGGL(k_again_same, dim3(nwg), dim3(256), 0, 0, buf, out, chunk); }
                        else { hipLaunchKernelGGL(k_again_shifted, dim3(nwg), dim3(256), 0, 0, buf, out, chunk); }
                        TRY(hipEventRecord(e1, 0));
                        TRY(hipEventSynchronize(e1));
                        float ms = 0.f;
                        TRY(hipEventElapsedTime(&ms, e0, e1));
                        (form == 0 ? same : shifted).push_back(ms * 1e3f);
                }
        }
        TRY(hipGetLastError());
        std::sort(same.begin(), same.end());
        std::sort(shifted.begin(), shifted.end());
        printf("{\"probe\": \"l2_carry\", \"bytes\": %zu, \"rounds\": %d, \"again_same_us\": {\"min\": %.2f, \"median\": %.2f}, "
               "\"again_shifted_us\": {\"min\": %.2f, \"median\": %.2f}}\n",
               bytes, rounds, same.front(), same[same.size() / 2], shifted.front(), shifted[shifted.size() / 2]);
        return 0;
}
