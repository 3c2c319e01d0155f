// common.hip.h — error reporting, device-buffer helpers, launch / workspace arithmetic and the dtype / precision dispatch shared by the
// C ABI sources.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>

#include "../../include/zett_hip.h"
#include "elem.hip.h"

namespace zett {

inline thread_local std::string g_err;

inline int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess)                                                                       \
            return ::zett::fail(ZETT_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// Every ABI entry point works on its handle's device and leaves the calling thread's current device as it found it
// (the caller may be a torch process holding several GPUs; zett_destroy can run from a garbage collector).
struct DeviceScope {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) err = hipSetDevice(device); else prev = -1;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};
#define ZETT_ON_DEVICE(dev)                                                                          \
    ::zett::DeviceScope _scope(dev);                                                                 \
    if (_scope.err != hipSuccess) return ::zett::fail(ZETT_E_HIP, "hipSetDevice(%d) failed: %s", (int)(dev), hipGetErrorString(_scope.err))

struct DevBuf {   // grow-only device allocation, freed with its owner
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int reserve(size_t need) {
        if (need <= bytes) return 0;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        need = (need + 255) & ~(size_t)255;
        hipError_t e = hipMalloc(&p, need);
        if (e != hipSuccess) return fail(ZETT_E_HIP, "hipMalloc(%zu) failed: %s", need, hipGetErrorString(e));
        bytes = need;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <typename U> U* as() const { return (U*)p; }
};

// ---- launch and workspace arithmetic of the entry points ---------------------------------------------------------------------
inline bool aligned(const void* p, size_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }          // bytes: a power of two
// a grid of `workgroups` workgroups, at least 1 and at most `most` (the kernel strides over what a capped grid leaves)
inline int grid_for(int64_t workgroups, int64_t most) { return (int)std::max<int64_t>(1, std::min<int64_t>(workgroups, most)); }
inline int grid256(int64_t items, int64_t most) { return grid_for((items + 255) / 256, most); }           // 256 items per workgroup
// a workspace carved into arrays that each start on a 16-byte boundary: take(n) is the offset of the next n bytes
struct Carve {
    int64_t bytes = 0;
    int64_t take(int64_t n) { const int64_t at = bytes; bytes += (n + 15) & ~(int64_t)15; return at; }
};

// ---- runtime type codes as compile-time types --------------------------------------------------------------------------------
// zett_dtype -> storage type
template <int DT> struct Elem;
template <> struct Elem<ZETT_F32> { using type = float; };
template <> struct Elem<ZETT_F16> { using type = f16_t; };
template <> struct Elem<ZETT_BF16> { using type = bf16_t; };
template <int DT> using elem_t = typename Elem<DT>::type;

inline bool is_dtype(int32_t d) { return d == ZETT_F32 || d == ZETT_F16 || d == ZETT_BF16; }

// f(std::integral_constant<int, dtype>{}): a checked (is_dtype) runtime dtype code as a compile-time constant, e.g.
//     with_dtype(d, [&](auto dt) { hipLaunchKernelGGL((kernel<decltype(dt)::value>), ...); });
template <typename F> inline void with_dtype(int32_t dtype, F&& f) {
    if (dtype == ZETT_F32) f(std::integral_constant<int, ZETT_F32>{});
    else if (dtype == ZETT_F16) f(std::integral_constant<int, ZETT_F16>{});
    else f(std::integral_constant<int, ZETT_BF16>{});
}

// f(Arith<T>{}) with T the operand type of a zett_precision (checked by zett_create); returns what f returns, e.g.
//     return with_precision(h->precision, [&](auto a) { return do_forward<typename decltype(a)::type>(...); });
template <typename T> struct Arith { using type = T; };
template <typename F> inline auto with_precision(int precision, F&& f) {
    if (precision == ZETT_PREC_F16) return f(Arith<f16_t>{});
    if (precision == ZETT_PREC_BF16) return f(Arith<bf16_t>{});
    return f(Arith<float>{});
}

// The options of a handle that decide how one GEMM of the forward is launched (zett_set_option names; defaults of zett_create):
// plain integers, kept here so that the handle can hold them without seeing a GEMM header (gemm_launch.hip.h reads them).
struct GemmOptions {
    int gemm_variant = 0;         // 0 auto, else the tile every launch that can takes: 1 = 128x128, 2 = 256x256 register-staged (8 waves),
                                  // 3 = 384x256 LDS-DMA, 7 = 256x256 four-wave direct-to-LDS, 8 = as 7 with the generic epilogue drain
    int gemm4d_min_k = 512;       // 16-bit launches with K >= this take the four-wave direct-to-LDS tile (r2: with the streamlined epilogues it is
                                  // ahead of gemm8r down to K = 768: +1.8 % on the XLM-R workload)
    int gemm_tail_split = 1;      // gemm4d: a launch's partly filled last round of 256 CUs as 128x256 tiles (gemm4d.hip.h gemm4d_row_split): 0 never,
                                  // 1 when the split is cheaper (default), 2 = cut every launch in the middle, 3 = half tiles only (tests: same bits)
    int gemm_tile_order = 0;      // gemm4d: 0 = column-tile-major groups, 1 = row-tile-major groups (A/B)
    int gemm_group = 0;           // gemm4d: column (order 0) / row (order 1) tiles per group; 0 = the kernel's default, 4 (A/B)
};

}  // namespace zett
