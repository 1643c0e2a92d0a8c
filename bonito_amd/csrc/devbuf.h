// Host-side helpers shared by engine.cpp and abi.cpp: an owning device buffer, fp16 uploads, convolution lengths.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "common.h"

namespace {      // (internal to each translation unit that includes this)

// fp32 -> fp16 bits, round-to-nearest-even (host)
static inline uint16_t f2h(float f) {
    _Float16 h = (_Float16)f;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

static inline int conv_out_len(int L, int K, int stride, int pad) { return (L + 2 * pad - K) / stride + 1; }

// Device memory that frees itself. The destructor runs hipFree on the device that is current then: owners that live on another
// device than the caller's make theirs current first (bh_encoder_destroy).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    int alloc(size_t n) {
        release();
        bytes = n;
        if (n == 0) return 0;
        BH_CHECK_HIP(hipMalloc(&p, n));
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
};

static inline int upload(DevBuf& b, const void* host, size_t bytes) {
    if (b.alloc(bytes)) return -1;
    BH_CHECK_HIP(hipMemcpy(b.p, host, bytes, hipMemcpyHostToDevice));
    return 0;
}
static inline int upload_f16(DevBuf& b, const float* w, size_t n) {
    std::vector<uint16_t> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = f2h(w[i]);
    return upload(b, h.data(), n * 2);
}
static inline int upload_f32(DevBuf& b, const float* w, size_t n) { return upload(b, w, n * 4); }

}  // namespace
