// jpeg2png_amd — the table estimator's device half: j2p_samples_histogram, the histogram of the step-1 coefficient magnitudes
// of a channel's 8-bit samples (include/jpeg2png_amd.h, "Estimated tables").  A translation unit of its own: the kernel shares
// j2p_dct.hip.h with the solver's and the output stage's, and nothing it does changes theirs.  The estimator itself is host C
// (j2p_quant_estimate.h, compute_host.c).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "jpeg2png_amd.h"
#include "j2p_internal.h"
#include "j2p_hip_host.h"
#include "j2p_estimate_kernels.hip.h"

using namespace j2p;

namespace {

constexpr size_t kHistBytes = 64 * (size_t)kHistBins * sizeof(uint32_t), kCountsBytes = 64;     // (two counters, padded)

// a pooled device block for the length of one call
struct PoolBlock {
        int device;
        void *ptr = nullptr;
        size_t got = 0;
        explicit PoolBlock(int dev) : device(dev) {}
        ~PoolBlock()
        {
                if(ptr) { j2p_pool_give(device, ptr, got); }
        }
};

// everything queued on `stream`: the zeroed histogram, the staged samples (host memory: the staging rule of sample input —
// rows of (w - 1) * stride_x + 1 bytes at a pitch that keeps every row 8-byte aligned, one 2-D copy), the kernel, the copy back
int histogram(int device, hipStream_t stream, j2p_samples m, bool on_device, PoolBlock &block, uint32_t *hist_host, unsigned long long counts_host[2])
{
        const unsigned blocks_w = m.w / 8, block_rows = m.h / 8;
        const size_t row_bytes = (size_t)(blocks_w * 8 - 1) * (size_t)m.stride_x + 1, pitch = (row_bytes + 7) & ~(size_t)7;
        const size_t stage_bytes = on_device ? 0 : pitch * block_rows * 8;
        HIP_TRY(j2p_pool_take(device, kHistBytes + kCountsBytes + stage_bytes, &block.ptr, &block.got));
        uint8_t *base = static_cast<uint8_t *>(block.ptr);
        uint32_t *hist = reinterpret_cast<uint32_t *>(base);
        unsigned long long *counts = reinterpret_cast<unsigned long long *>(base + kHistBytes);
        HIP_TRY(hipMemsetAsync(base, 0, kHistBytes + kCountsBytes, stream));
        if(!on_device) {
                uint8_t *stage = base + kHistBytes + kCountsBytes;
                if((size_t)m.stride_y >= row_bytes) {
                        HIP_TRY(hipMemcpy2DAsync(stage, pitch, m.data, (size_t)m.stride_y, row_bytes, block_rows * 8, hipMemcpyHostToDevice, stream));
                } else {
                        // (rows that overlap in memory: no 2-D copy describes them)
                        for(unsigned y = 0; y < block_rows * 8; y++) {
                                HIP_TRY(hipMemcpyAsync(stage + y * pitch, m.data + (size_t)y * (size_t)m.stride_y, row_bytes, hipMemcpyHostToDevice, stream));
                        }
                }
                m.data = stage;
                m.stride_y = (ptrdiff_t)pitch;
        }
        const unsigned long long groups = (unsigned long long)((blocks_w + 7) / 8) * block_rows;
        const unsigned long long need = (groups + 3) / 4;
        const unsigned grid = need < kHistMaxWorkgroups ? (unsigned)need : kHistMaxWorkgroups;
        const int wide = m.stride_x == 1 && ((reinterpret_cast<uintptr_t>(m.data) | (uintptr_t)m.stride_y) & 7) == 0;
        hipLaunchKernelGGL(k_samples_dct_histogram, dim3(grid), dim3(256), 0, stream, m.data, m.stride_y, m.stride_x, wide, blocks_w, block_rows, hist,
                           counts);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(hist_host, hist, kHistBytes, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(counts_host, counts, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return J2P_OK;
}

}  // namespace

extern "C" int j2p_samples_histogram(int device, void *stream, const j2p_samples *samples, uint32_t *hist_host, unsigned long long *blocks,
                                     unsigned long long *excluded)
{
        if(!samples || !hist_host || !blocks || !excluded) { return j2p_fail(J2P_EINVAL, "j2p_samples_histogram: NULL argument"); }
        const j2p_samples m = *samples;
        if(!m.data) { return j2p_fail(J2P_EINVAL, "samples: data is NULL"); }
        if(m.w == 0 || m.h == 0) { return j2p_fail(J2P_EINVAL, "samples: %ux%u samples", m.w, m.h); }
        if(m.stride_y < 1 || m.stride_x < 1) { return j2p_fail(J2P_EINVAL, "samples: strides (y, x) = (%td, %td) must be at least 1", m.stride_y, m.stride_x); }
        int ndev = 0;
        if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
                return j2p_fail(J2P_EDEVICE, "no HIP device available: the histogram has no CPU fallback");
        }
        if(device < 0 || device >= ndev) { return j2p_fail(J2P_EINVAL, "device %d out of range (0..%d)", device, ndev - 1); }
        DeviceGuard guard(device);
        if(!guard.ok) { return j2p_fail(J2P_EDEVICE, "hipSetDevice(%d) failed", device); }
        int where = -1;
        const int kind = j2p_memory_of_pointer(m.data, &where);
        if(kind == J2P_MEMORY_OTHER || (kind == J2P_MEMORY_DEVICE && where != device)) {
                return j2p_fail(J2P_EINVAL, "samples: data is neither host memory nor device memory of device %d (managed memory and other GPUs' are refused)", device);
        }
        memset(hist_host, 0, kHistBytes);
        *blocks = *excluded = 0;
        if(m.w < 8 || m.h < 8) { return J2P_OK; }             // no complete block: nothing to launch
        if((unsigned long long)((m.w / 8 + 7) / 8) * (m.h / 8) >= (1ull << 31)) { return j2p_fail(J2P_EINVAL, "samples: %ux%u samples are more than the histogram takes", m.w, m.h); }
        hipStream_t st = (hipStream_t)stream;
        bool own = false;
        if(!st) {
                HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
                own = true;
        }
        unsigned long long counts[2] = {0, 0};
        int rc;
        {
                PoolBlock block(device);
                rc = histogram(device, st, m, kind == J2P_MEMORY_DEVICE, block, hist_host, counts);
                // (a failure may have left work queued that reads the block)
                if(rc != J2P_OK) { (void)hipStreamSynchronize(st); }
        }
        if(own) { (void)hipStreamDestroy(st); }
        if(rc != J2P_OK) { return rc; }
        *blocks = counts[0];
        *excluded = counts[1];
        return J2P_OK;
}
