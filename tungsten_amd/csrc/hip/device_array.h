// DeviceArray<T>: the one owner of a device array -- pointer and capacity together, freed by the destructor, never copied.  The members of tghip_ctx
// (shim_context.h) that grow on demand, its words allocated once, and the per-call arrays of tghip_trace_rays / tghip_debug_* are of this type: an
// early return frees what the call allocated, and `delete ctx` -- the last thing tghip_destroy does, with the context's device current and every
// stream idle -- frees what the context held.  (DeviceBuffers, shim_context.h, is the other thing: many arrays of one upload freed together.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "../../../include/tungsten_hip.h"

// A failed HIP call ends the calling function with TGHIP_E_HIP and its text in (ctx)->error
#define HIP_TRY(ctx, call)                                                                  \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            (ctx)->error = std::string(#call) + ": " + hipGetErrorString(e_);               \
            return TGHIP_E_HIP;                                                             \
        }                                                                                   \
    } while (0)

template<typename T>
class DeviceArray {
public:
    DeviceArray() = default;
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
    ~DeviceArray() { release(); }

    T *get() const { return dev; }
    explicit operator bool() const { return dev != nullptr; }
    void release() { if (dev) (void)hipFree(dev); dev = nullptr; cap = 0; }

    // Room for `need` elements: grows on demand and never shrinks.  The old contents are dropped.  An allocation is never empty: it happens only for
    // need > cap >= 0 (*reallocated says whether one did).  A failed one leaves the array empty and its text in ctx->error.
    template<typename Ctx>
    int grow(Ctx *ctx, size_t need, bool *reallocated = nullptr)
    {
        if (reallocated) *reallocated = false;
        if (cap >= need) return TGHIP_OK;
        release();
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&dev), need*sizeof(T)));
        cap = need;
        if (reallocated) *reallocated = true;
        return TGHIP_OK;
    }
    // `count` elements allocated the first time only (a word the kernels poll, a counter: 64 bytes that stay where they are)
    hipError_t once(size_t count)
    {
        if (dev) return hipSuccess;
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&dev), count*sizeof(T));
        if (e == hipSuccess) cap = count; else dev = nullptr;
        return e;
    }

private:
    T *dev = nullptr;
    size_t cap = 0;
};
