// mem_check.cpp -- the owners of pypevoc_amd/csrc/pvx_mem.h against a fake allocator, on the CPU (tests/test_mem_cpu.py
// builds this with the host compiler and -fsanitize=address,undefined; no GPU library is linked).  The fakes below stand in
// for hipMalloc / hipFree / hipHostMalloc / hipHostFree: malloc-backed, they count calls, record sizes and can be told to fail
// the next allocations.  A double free or a leak is the sanitizer's to report.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <utility>
#include <vector>

#include "pvx_mem.h"

static int n_alloc = 0, n_free = 0, fail_next = 0;
static std::vector<size_t> sizes;          // of every allocation attempt, failed ones included
static std::vector<char> order;            // 'a' / 'f' in call order
static char last_error[256] = "";

static hipError_t fake_alloc(void** p, size_t n) {
    n_alloc++; sizes.push_back(n); order.push_back('a');
    if (fail_next > 0) { fail_next--; *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(n);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
static hipError_t fake_free(void* p) { n_free++; order.push_back('f'); free(p); return hipSuccess; }

extern "C" hipError_t hipMalloc(void** p, size_t n) { return fake_alloc(p, n); }
extern "C" hipError_t hipFree(void* p) { return fake_free(p); }
extern "C" hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { return fake_alloc(p, n); }
extern "C" hipError_t hipHostFree(void* p) { return fake_free(p); }
void pvx_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
}

static int failures = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static void reset_counts() { n_alloc = n_free = fail_next = 0; sizes.clear(); order.clear(); last_error[0] = 0; }

template <class M> static void check_owner(const char* alloc_name) {
    // an empty object: nothing to free
    reset_counts();
    { M m; CHECK(!m && m.cap() == 0 && m.get() == nullptr); }
    CHECK(n_alloc == 0 && n_free == 0);

    // grow below capacity keeps the pointer and makes no call; above it frees exactly once, before it allocates
    reset_counts();
    {
        M m;
        CHECK(m.grow(1000, Sizing::exact) == PVX_OK && m.cap() == 1000 && n_alloc == 1 && n_free == 0 && sizes.back() == 1000);
        void* const p0 = m.get();
        CHECK(m.grow(1000, Sizing::exact) == PVX_OK && m.grow(1, Sizing::headroom) == PVX_OK && m.grow(0, Sizing::exact) == PVX_OK);
        CHECK(m.get() == p0 && m.cap() == 1000 && n_alloc == 1 && n_free == 0);
        CHECK(m.grow(1001, Sizing::exact) == PVX_OK && m.cap() == 1001);
        CHECK(n_alloc == 2 && n_free == 1 && order.size() == 3 && order[1] == 'f' && order[2] == 'a');
    }
    CHECK(n_alloc == 2 && n_free == 2);

    // the headroom policy: need + need/4 + 256; when that fails, exactly `need`
    reset_counts();
    {
        M m;
        CHECK(m.grow(4000, Sizing::headroom) == PVX_OK && m.cap() == 4000 + 1000 + 256 && n_alloc == 1 && sizes[0] == 5256);
        CHECK(m.grow(5256, Sizing::headroom) == PVX_OK && n_alloc == 1);
        fail_next = 1;
        CHECK(m.grow(8000, Sizing::headroom) == PVX_OK && m.cap() == 8000 && m);
        CHECK(n_alloc == 3 && n_free == 1 && sizes[1] == 8000 + 2000 + 256 && sizes[2] == 8000);
        CHECK(order[1] == 'f');                                    // the old buffer went before either attempt
        // both fail: empty, capacity 0, PVX_ERR_ALLOC and the message
        fail_next = 2;
        CHECK(m.grow(9000, Sizing::headroom) == PVX_ERR_ALLOC && !m && m.cap() == 0 && m.get() == nullptr);
        CHECK(n_alloc == 5 && n_free == 2 && sizes[3] == 9000 + 2250 + 256 && sizes[4] == 9000);
        char want[64];
        snprintf(want, sizeof(want), "%s(9000) failed", alloc_name);
        CHECK(std::string(last_error) == want);
    }
    CHECK(n_free == 2);                                            // the destructor of the emptied object made no call

    // exact sizing makes one attempt; alloc() replaces what the object held; 0 bytes hold one byte at capacity 0
    reset_counts();
    {
        M m;
        fail_next = 1;
        CHECK(m.grow(100, Sizing::exact) == PVX_ERR_ALLOC && n_alloc == 1 && !m);
        CHECK(m.alloc(64) == PVX_OK && m.cap() == 64 && m.alloc(32) == PVX_OK && m.cap() == 32 && n_alloc == 3 && n_free == 1);
        CHECK(m.alloc(0) == PVX_OK && m && m.cap() == 0 && sizes.back() == 1);
        m.reset();
        CHECK(!m && n_free == 3);
    }
    CHECK(n_alloc == 4 && n_free == 3);

    // moves: one owner at a time, no double free
    reset_counts();
    {
        M a;
        CHECK(a.alloc(10) == PVX_OK);
        void* const pa = a.get();
        M b(std::move(a));
        CHECK(!a && a.cap() == 0 && b.get() == pa && b.cap() == 10);
        M c;
        CHECK(c.alloc(20) == PVX_OK);
        c = std::move(b);                                          // frees c's own buffer, takes b's
        CHECK(!b && c.get() == pa && c.cap() == 10 && n_free == 1);
        M& self = c;
        c = std::move(self);
        CHECK(c.get() == pa && n_free == 1);
        std::vector<M> v;
        v.push_back(std::move(c));
        v.emplace_back();
        CHECK(v[0].get() == pa && n_free == 1);
    }
    CHECK(n_alloc == 2 && n_free == 2);
}

int main() {
    check_owner<DevMem>("hipMalloc");
    check_owner<PinMem>("hipHostMalloc");
    if (failures) { fprintf(stderr, "mem_check: %d checks failed\n", failures); return 1; }
    printf("mem_check ok\n");
    return 0;
}
