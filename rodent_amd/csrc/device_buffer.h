// device_buffer.h -- host-side helpers shared by the HIP sources: HIP_CHECK and the grow-only device arrays of the launch contexts.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstdlib>

#define HIP_CHECK(expr)                                                                       \
    do {                                                                                      \
        hipError_t err_ = (expr);                                                             \
        if (err_ != hipSuccess) {                                                             \
            fprintf(stderr, "rodent_hip: %s failed: %s (%s:%d)\n", #expr,                     \
                    hipGetErrorString(err_), __FILE__, __LINE__);                             \
            abort();                                                                          \
        }                                                                                     \
    } while (0)

constexpr int kNoFill = -1;

// A device array that only grows: ensure(n) leaves it alone when it holds n elements already; otherwise it waits for the device (work in
// flight may still read the old block), frees the old block and allocates exactly n elements, byte-filled with `fill` unless that is
// kNoFill.  The caller rounds n, and keeps whatever it enqueues with the pointer under the lock that guards the buffer.  Nothing is freed
// on destruction: the contexts that own these live until process exit, when the HIP runtime may already be gone.
template <typename T> struct DeviceBuffer {
    T* ptr = nullptr;
    size_t count = 0;

    T* ensure(size_t n, int fill = kNoFill) { return grow(n, fill, false); }
    // the same, but a device without room for n elements leaves the buffer empty (ptr == nullptr) instead of aborting
    T* try_ensure(size_t n, int fill) { return grow(n, fill, true); }

private:
    T* grow(size_t n, int fill, bool may_fail) {
        if (n <= count) return ptr;
        if (ptr) { HIP_CHECK(hipDeviceSynchronize()); HIP_CHECK(hipFree(ptr)); }
        ptr = nullptr; count = 0;
        if (!may_fail) HIP_CHECK(hipMalloc(&ptr, sizeof(T) * n));
        else if (hipMalloc(&ptr, sizeof(T) * n) != hipSuccess) { (void)hipGetLastError(); ptr = nullptr; return nullptr; }
        // The fill runs on the null stream and does not wait for the host; a stream created non-blocking does not wait for the null
        // stream either, so a kernel enqueued there right after ensure() could run before (or while) the block is filled -- the first
        // "sorted" launch of a fresh context counted into sort_totals and had its counts zeroed under it.  Wait for the fill here.
        if (fill != kNoFill) { HIP_CHECK(hipMemset(ptr, fill, sizeof(T) * n)); HIP_CHECK(hipStreamSynchronize(nullptr)); }
        count = n;
        return ptr;
    }
};
