// jpeg2png_amd — the device-memory pool and the per-device table of live bytes (j2p_internal.h).  Host code only.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <mutex>
#include <vector>

#include "jpeg2png_amd.h"
#include "j2p_internal.h"
#include "j2p_hip_host.h"

namespace {

// ---------------------------------------------------------------------------
// Device-memory pool.  hipMalloc / hipFree cost milliseconds and hipFree synchronises the whole device, which
// serialises the concurrent compute() calls of a multi-threaded host (jpeg2png.c:147,330) far more than the
// solves themselves at 1080p.  A solver therefore makes ONE allocation (its arena) and returns it here when it
// is destroyed; the next solver on that device takes the smallest cached block that fits.  Bounded: at most
// kPoolBlocks blocks / kPoolBytes bytes stay cached per process, the rest is released; j2p_pool_trim() drops all.
// ---------------------------------------------------------------------------
struct PoolBlock {
        int device;
        void *ptr;
        size_t bytes;
};
std::mutex g_pool_lock;
std::vector<PoolBlock> g_pool;
thread_local unsigned long long t_pool_takes = 0;      // j2p_pool_thread_takes: this thread's calls of j2p_pool_take
constexpr size_t kPoolBlocks = 16;                     // per device
constexpr size_t kPoolBytesDefault = (size_t)8 << 30;  // per device; J2P_POOL_MIB overrides (0 = no caching)

size_t pool_cap_bytes()
{
        static const size_t cap = [] {
                const char *env = getenv("J2P_POOL_MIB");
                if(env && *env) { return (size_t)strtoull(env, nullptr, 10) << 20; }
                return kPoolBytesDefault;
        }();
        return cap;
}

void pool_drop_all()
{
        std::vector<PoolBlock> drop;
        {
                std::lock_guard<std::mutex> g(g_pool_lock);
                drop.swap(g_pool);
        }
        for(const PoolBlock &b : drop) {
                DeviceGuard guard(b.device);
                (void)hipFree(b.ptr);
        }
}

}  // namespace

// hipMalloc for everything that does not go through the pool (log buffers, the stand-alone decode / DCT calls):
// on out-of-memory the cached arenas go back to the device and the allocation is tried once more
hipError_t j2p_dev_malloc(void **out, size_t bytes)
{
        hipError_t e = hipMalloc(out, bytes);
        if(e == hipErrorOutOfMemory) {
                (void)hipGetLastError();
                pool_drop_all();
                e = hipMalloc(out, bytes);
        }
        return e;
}

hipError_t j2p_pool_take(int device, size_t bytes, void **out, size_t *got)
{
        t_pool_takes++;
        {
                std::lock_guard<std::mutex> g(g_pool_lock);
                size_t best = g_pool.size();
                for(size_t i = 0; i < g_pool.size(); i++) {
                        const PoolBlock &b = g_pool[i];
                        // a block more than twice the size asked for stays for a larger customer
                        if(b.device == device && b.bytes >= bytes && b.bytes <= 2 * bytes + (1u << 20) &&
                           (best == g_pool.size() || b.bytes < g_pool[best].bytes)) { best = i; }
                }
                if(best != g_pool.size()) {
                        *out = g_pool[best].ptr;
                        *got = g_pool[best].bytes;
                        g_pool.erase(g_pool.begin() + (ptrdiff_t)best);
                        return hipSuccess;
                }
        }
        *got = bytes;
        return j2p_dev_malloc(out, bytes);
}

void j2p_pool_give(int device, void *ptr, size_t bytes)
{
        if(!ptr) { return; }
        {
                std::lock_guard<std::mutex> g(g_pool_lock);
                size_t total = bytes, blocks = 0;
                for(const PoolBlock &b : g_pool) {
                        if(b.device == device) { total += b.bytes; blocks++; }
                }
                if(blocks < kPoolBlocks && total <= pool_cap_bytes()) {
                        g_pool.push_back(PoolBlock{device, ptr, bytes});
                        return;
                }
        }
        (void)hipFree(ptr);
}

extern "C" void j2p_pool_trim(void) { pool_drop_all(); }
extern "C" unsigned long long j2p_pool_thread_takes(void) { return t_pool_takes; }

namespace {

constexpr int kMaxDevices = 64;
LiveBytes g_live[kMaxDevices];          // guarded by g_pool_lock

}  // namespace

void j2p_live_add(int device, const LiveBytes &b, int sign)
{
        if(device < 0 || device >= kMaxDevices) { return; }
        std::lock_guard<std::mutex> g(g_pool_lock);
        LiveBytes &l = g_live[device];
        if(sign > 0) { l.working_set += b.working_set; l.g += b.g; l.planes += b.planes; l.d += b.d; }
        else { l.working_set -= b.working_set; l.g -= b.g; l.planes -= b.planes; l.d -= b.d; }
}
LiveBytes j2p_live_on(int device)
{
        if(device < 0 || device >= kMaxDevices) { return LiveBytes{}; }
        std::lock_guard<std::mutex> g(g_pool_lock);
        return g_live[device];
}
