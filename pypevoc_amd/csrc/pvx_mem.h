// pvx_mem.h -- host only: move-only owners of what the host layer allocates (device and page-locked memory, events, streams,
// a real rocFFT plan, forward or inverse).  A destructor releases what its object holds; a failed step leaves the object empty.
//
// Workspaces that live as long as the process (PeriodWs, FbankWs, the plan-less tracker's and the process-wide staging
// rings; k_synth.hip's per-stream map holds raw pointers) are heap objects that are never deleted: they may have these owners
// as members, but no owner may sit in an object with static storage -- no HIP call may run from a destructor at process exit,
// when the runtime may already be gone.
#pragma once
#include <stddef.h>

#include <utility>

#include <hip/hip_runtime_api.h>
#include <rocfft/rocfft.h>

#include "pvx.h"

void pvx_set_error(const char* fmt, ...);

// how grow() sizes a new buffer: exactly what is asked for, or need + need/4 + 256 with a second try at exactly `need`
enum class Sizing { exact, headroom };

struct DevAlloc {
    static hipError_t get(void** p, size_t n) { return hipMalloc(p, n); }
    static void put(void* p) { (void)hipFree(p); }
    static const char* name() { return "hipMalloc"; }
};
struct PinAlloc {
    static hipError_t get(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
    static void put(void* p) { (void)hipHostFree(p); }
    static const char* name() { return "hipHostMalloc"; }
};

// a buffer and its capacity in bytes (what was asked for: a request of 0 bytes holds one byte at capacity 0)
template <class A> class Mem {
    void* p_ = nullptr;
    size_t cap_ = 0;
    bool take(size_t bytes) {
        if (A::get(&p_, bytes ? bytes : 1) != hipSuccess) { p_ = nullptr; return false; }
        cap_ = bytes;
        return true;
    }
public:
    Mem() = default;
    Mem(Mem&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Mem& operator=(Mem&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~Mem() { reset(); }
    void reset() { if (p_) A::put(p_); p_ = nullptr; cap_ = 0; }
    explicit operator bool() const { return p_ != nullptr; }
    void* get() const { return p_; }
    template <typename T> T* as() const { return (T*)p_; }
    size_t cap() const { return cap_; }
    // a buffer of exactly `bytes` (what it held before is freed first)
    int alloc(size_t bytes) { return grow_to(bytes, bytes, Sizing::exact); }
    // grow-only: keeps the buffer while need <= cap(); otherwise frees it, then allocates by `how`
    int grow(size_t need, Sizing how) { return p_ && need <= cap_ ? PVX_OK : grow_to(need, need + need / 4 + 256, how); }
private:
    int grow_to(size_t need, size_t roomy, Sizing how) {
        reset();
        if ((how == Sizing::headroom && take(roomy)) || take(need)) return PVX_OK;
        pvx_set_error("%s(%zu) failed", A::name(), need);
        return PVX_ERR_ALLOC;
    }
};
using DevMem = Mem<DevAlloc>;
using PinMem = Mem<PinAlloc>;

// an event or a stream, created on first use (ensure) with the flags of that call
template <class H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)> class Handle {
    H h_ = nullptr;
public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
        return *this;
    }
    ~Handle() { reset(); }
    void reset() { if (h_) (void)Destroy(h_); h_ = nullptr; }
    hipError_t ensure(unsigned flags) { return h_ ? hipSuccess : Create(&h_, flags); }
    operator H() const { return h_; }
};
using Event = Handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

// A batched 1-D real -> Hermitian-interleaved rocFFT plan (create), or its inverse (create_inverse), with its execution info.
// `work` is the plan's own work buffer, for the callers that do not share one between plans or keep it beyond a plan; either
// kind reaches the plan through set_work().
class RealFft {
    rocfft_plan plan_ = nullptr;
    rocfft_execution_info info_ = nullptr;
    size_t work_bytes_ = 0;
public:
    DevMem work;
    enum Step { done = 0, describe, plan, info };   // where create() failed (the callers word their own messages)
    RealFft() = default;
    RealFft(RealFft&& o) noexcept : plan_(o.plan_), info_(o.info_), work_bytes_(o.work_bytes_), work(std::move(o.work)) {
        o.plan_ = nullptr; o.info_ = nullptr; o.work_bytes_ = 0;
    }
    RealFft& operator=(RealFft&& o) noexcept {
        if (this != &o) {
            reset();
            plan_ = o.plan_; info_ = o.info_; work_bytes_ = o.work_bytes_; work = std::move(o.work);
            o.plan_ = nullptr; o.info_ = nullptr; o.work_bytes_ = 0;
        }
        return *this;
    }
    ~RealFft() { reset(); }
    void reset() {
        if (info_) (void)rocfft_execution_info_destroy(info_);
        if (plan_) (void)rocfft_plan_destroy(plan_);
        info_ = nullptr; plan_ = nullptr; work_bytes_ = 0;
        work.reset();
    }
    explicit operator bool() const { return plan_ != nullptr; }
    size_t work_bytes() const { return work_bytes_; }
    // `batch` transforms of `len` reals, idist reals / odist complex values apart; on failure the object is empty and *st says why
    Step create(size_t len, size_t batch, rocfft_precision precision, rocfft_result_placement placement, size_t idist, size_t odist,
                rocfft_status* st) {
        return make(false, len, batch, precision, placement, idist, odist, st);
    }
    // the inverse sibling: `batch` Hermitian-interleaved half spectra of len/2 + 1 complex values, idist complex values apart, to
    // `len` reals each, odist reals apart, unscaled (the caller divides by len).  rocFFT may overwrite the spectra it reads
    Step create_inverse(size_t len, size_t batch, rocfft_precision precision, rocfft_result_placement placement, size_t idist,
                        size_t odist, rocfft_status* st) {
        return make(true, len, batch, precision, placement, idist, odist, st);
    }
private:
    Step make(bool inverse, size_t len, size_t batch, rocfft_precision precision, rocfft_result_placement placement, size_t idist,
              size_t odist, rocfft_status* st) {
        reset();
        rocfft_plan_description desc = nullptr;
        if ((*st = rocfft_plan_description_create(&desc)) != rocfft_status_success) return describe;
        size_t istride = 1, ostride = 1;
        *st = rocfft_plan_description_set_data_layout(desc, inverse ? rocfft_array_type_hermitian_interleaved : rocfft_array_type_real,
                                                      inverse ? rocfft_array_type_real : rocfft_array_type_hermitian_interleaved, nullptr,
                                                      nullptr, 1, &istride, idist, 1, &ostride, odist);
        if (*st == rocfft_status_success)
            *st = rocfft_plan_create(&plan_, placement, inverse ? rocfft_transform_type_real_inverse : rocfft_transform_type_real_forward,
                                     precision, 1, &len, batch, desc);
        (void)rocfft_plan_description_destroy(desc);
        if (*st != rocfft_status_success) { plan_ = nullptr; return plan; }
        if ((*st = rocfft_plan_get_work_buffer_size(plan_, &work_bytes_)) == rocfft_status_success) *st = rocfft_execution_info_create(&info_);
        if (*st != rocfft_status_success) { info_ = nullptr; reset(); return info; }
        return done;
    }
public:
    rocfft_status set_work(void* buf, size_t bytes) { return rocfft_execution_info_set_work_buffer(info_, buf, bytes); }
    rocfft_status execute(void* in, void* out, hipStream_t s) {
        const rocfft_status st = rocfft_execution_info_set_stream(info_, s);
        return st != rocfft_status_success ? st : rocfft_execute(plan_, &in, &out, info_);
    }
};
