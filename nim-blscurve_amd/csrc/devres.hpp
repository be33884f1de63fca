// Owners of the host layer's HIP resources: device buffers, events, streams, pinned host memory.  Host-only; included by host_api.inc
// (same translation unit: g_err and the error codes are in scope).  Each owner is move-only, converts to the raw handle the HIP calls and
// kernel launches take, and releases in its destructor.  Nothing else in the host layer creates or releases such a resource.
#pragma once
#include <memory>
#include <utility>

// owned objects alive in the process (mi355_bls_debug_live_resources): up on every successful creation, down on every release
static std::atomic<int> g_live_resources{0};

template <class T>
struct dev_buf {
    T* p = nullptr;
    size_t bytes = 0;
    dev_buf() = default;
    dev_buf(dev_buf&& o) noexcept { swap(o); }
    dev_buf& operator=(dev_buf&& o) noexcept {
        if (this != &o) reset(), swap(o);
        return *this;
    }
    ~dev_buf() { reset(); }
    operator T*() const { return p; }
    void swap(dev_buf& o) noexcept { std::swap(p, o.p), std::swap(bytes, o.bytes); }
    void reset() {
        if (p) (void)hipFree(p), g_live_resources--;
        p = nullptr, bytes = 0;
    }
    // exactly n bytes; a failure leaves the buffer empty
    int alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc((void**)&p, n);
        if (e != hipSuccess) {
            p = nullptr;
            g_err = std::string("hipMalloc: ") + hipGetErrorString(e);
            return MI355_BLS_ERR_HIP;
        }
        if (p) bytes = n, g_live_resources++;
        return 0;
    }
    // at least n bytes: a buffer that is too small is released and n + slack allocated (the contents are not kept)
    int reserve(size_t n, size_t slack) { return n <= bytes ? 0 : alloc(n + slack); }
};

// A fixed-base window table (mi355_bls_p1s_table_create): the rows in device memory and the parameters they were made with.  It belongs to its
// caller, not to the context that made it: mi355_bls_p1s_table_destroy releases it, on its own device.
struct mi355_bls_p1s_table {
    int device = 0;
    size_t npoints = 0;
    uint32_t wbits = 0, nbits = 0, nwin = 0;     // nwin = plan::fixed_nwin(wbits, nbits) rows of npoints entries
    dev_buf<uint32_t> rows;                      // entry w x npoints + i: k_pip_convert's 32-word record of [2^(w wbits)] P_i
    ~mi355_bls_p1s_table() {
        if (rows) (void)hipSetDevice(device);
    }
};

// The setup of the all-openings call (mi355_bls_fk20_setup_create): NTT_2n(s^) of csrc/fk20.hpp in device memory.  p1s_table's ownership:
// it belongs to its caller, mi355_bls_fk20_setup_destroy releases it, on its own device.
struct mi355_bls_fk20_setup {
    int device = 0;
    size_t n = 0;
    size_t cell = 1;                             // the cell size l the handle was made for (mi355_bls_fk20_setup_create_cells); 1: all openings
    dev_buf<uint32_t> x;                         // 2n canonical affine images (24 words each), slot s: entry rev_(m+1)(s) of the transform;
                                                 // cell > 1: image slot l + v is entry rev(slot) of NTT_2q(s^(v)) (csrc/fk20cells.hpp)
    ~mi355_bls_fk20_setup() {
        if (x) (void)hipSetDevice(device);
    }
};

// H: the handle; Destroy: what releases it
template <class H, hipError_t (*Destroy)(H)>
struct dev_handle {
    H h = nullptr;
    dev_handle() = default;
    dev_handle(dev_handle&& o) noexcept { swap(o); }
    dev_handle& operator=(dev_handle&& o) noexcept {
        if (this != &o) reset(), swap(o);
        return *this;
    }
    ~dev_handle() { reset(); }
    operator H() const { return h; }
    void swap(dev_handle& o) noexcept { std::swap(h, o.h); }
    void reset() {
        if (h) (void)Destroy(h), g_live_resources--;
        h = nullptr;
    }
};
struct dev_event : dev_handle<hipEvent_t, hipEventDestroy> {
    int create(unsigned flags = hipEventDefault) {
        reset();
        HIPCHK(hipEventCreateWithFlags(&h, flags));
        g_live_resources++;
        return 0;
    }
};
struct dev_stream : dev_handle<hipStream_t, hipStreamDestroy> {
    // a non-blocking stream; prio: at that priority where the runtime grants it, at the default one otherwise.  false: no stream.
    bool create(const int* prio = nullptr) {
        reset();
        if (prio && hipStreamCreateWithPriority(&h, hipStreamNonBlocking, *prio) != hipSuccess) (void)hipGetLastError(), h = nullptr;
        if (!h && hipStreamCreateWithFlags(&h, hipStreamNonBlocking) != hipSuccess) (void)hipGetLastError(), h = nullptr;
        if (h) g_live_resources++;
        return h != nullptr;
    }
};
// page-locked host words
static hipError_t pinned_free(uint32_t* p) { return hipHostFree(p); }
struct pinned_words : dev_handle<uint32_t*, pinned_free> {
    int alloc(size_t bytes) {
        reset();
        HIPCHK(hipHostMalloc((void**)&h, bytes, hipHostMallocDefault));
        g_live_resources++;
        return 0;
    }
};
