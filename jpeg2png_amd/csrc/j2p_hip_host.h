// jpeg2png_amd — host-side HIP helpers shared by the translation units that call the runtime with a solver's device and
// stream (j2p_solver.hip, j2p_output.hip, j2p_codec.hip); not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "j2p_internal.h"          // j2p_fail

// returns from the calling function with the error text set when a HIP call fails
#define HIP_TRY(expr)                                                                              \
        do {                                                                                       \
                hipError_t e_ = (expr);                                                            \
                if(e_ != hipSuccess) {                                                             \
                        return j2p_fail(e_ == hipErrorOutOfMemory ? J2P_ENOMEM : J2P_EDEVICE,      \
                                        "%s failed: %s", #expr, hipGetErrorString(e_));            \
                }                                                                                  \
        } while(0)

// makes `dev` the calling thread's device for a scope
struct DeviceGuard {
        int prev = -1;
        bool ok = true;
        explicit DeviceGuard(int dev)
        {
                if(hipGetDevice(&prev) != hipSuccess) { prev = -1; }
                if(prev != dev) { ok = hipSetDevice(dev) == hipSuccess; }
        }
        ~DeviceGuard()
        {
                if(prev >= 0) { (void)hipSetDevice(prev); }
        }
};
