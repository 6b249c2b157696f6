// pvx_host.h -- host only, internal (include/pvx.h does not include it): what pvx_ops.hip shares with pvx_api.hip.
#pragma once
#include <string.h>

#include "pvx_internal.h"
#include "pvx_mem.h"

// Transfers between the CALLER's arrays and device memory, through pvx_api.hip's staging: they return when the bytes have arrived.
int pvx_host_to_device(void* dev, const void* host, size_t bytes);
int pvx_device_to_host(void* host, const void* dev, size_t bytes);
// PVX_MAX_DEVICE_BYTES where it is set to a positive number, else `dflt`: the per-buffer budget that decides chunking
size_t pvx_device_bytes_limit(size_t dflt);
static inline size_t dtype_size(int x_dtype) { return x_dtype == PVX_F32 ? 4 : (x_dtype == PVX_F64 ? 8 : 2); }
// the calling thread's slot that pvx_jumps_last_kernels() reads (pvx_jump_select_resident sits beside the plan)
const char** pvx_jumps_kernels_slot();

// a host array on the device for the length of a call (nullptr stays nullptr)
struct Staged {
    DevMem mem;
    int put(const void* host, size_t bytes) {
        int rc;
        if (!host) return PVX_OK;
        if ((rc = mem.alloc(bytes ? bytes : 8)) != PVX_OK) return rc;
        return bytes ? pvx_host_to_device(mem.get(), host, bytes) : PVX_OK;
    }
    int room(size_t bytes) { return mem.alloc(bytes ? bytes : 8); }
    int get(void* host, size_t bytes) { return bytes ? pvx_device_to_host(host, mem.get(), bytes) : PVX_OK; }
    template <typename T> T* as() const { return mem.as<T>(); }
};

// rows of `bytes` each from a device buffer to the caller's: on the stream (DEV), or to the host before the return
template <bool DEV> static int rows_out(void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (!dst || bytes == 0) return PVX_OK;
    if (!DEV) return pvx_device_to_host(dst, src, bytes);
    PVX_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
    return PVX_OK;
}
template <bool DEV> static int zero_out(double* dst, int64_t count, hipStream_t s) {
    if (!dst || count <= 0) return PVX_OK;
    if (!DEV) { memset(dst, 0, (size_t)count * 8); return PVX_OK; }
    PVX_HIP_CHECK(hipMemsetAsync(dst, 0, (size_t)count * 8, s));
    return PVX_OK;
}
