// Host-side helpers shared by the C-ABI entry points: the error text, per-device one-time work
// and device properties. A process may drive several GPUs through the C-ABI (one device per thread, or a
// loop over devices), so nothing here is a per-process flag: kernel attributes are set once per
// device, the CU count is cached per device, and both are safe to call from several threads.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

namespace evxh {

inline int cur_device() {
    int d = 0;
    return hipGetDevice(&d) == hipSuccess ? d : -1;
}

// Runs f() unless it already ran for the current device (devices 0..63; beyond, every call runs
// it). Two threads may both run it the first time: f must be idempotent (attribute setters are).
template <class F>
inline void once_per_device(std::atomic<uint64_t>& done, F&& f) {
    const int d = cur_device();
    const uint64_t bit = (d >= 0 && d < 64) ? (1ull << d) : 0ull;
    if (bit && (done.load(std::memory_order_acquire) & bit)) return;
    f();
    if (bit) done.fetch_or(bit, std::memory_order_acq_rel);
}

// Raises a kernel's dynamic-LDS limit on the current device, once per device.
inline void max_lds_once(std::atomic<uint64_t>& done, const void* const* kernels, int n, int bytes) {
    once_per_device(done, [&] {
        for (int i = 0; i < n; i++) (void)hipFuncSetAttribute(kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    });
}

// The C-ABI's error text: the message of the calling thread's last failed call, whichever entry
// point it came from. evx_last_error() and the per-family getters all return this buffer.
inline thread_local char g_err[512] = "";

inline int fail(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

// fail() with a printf format: the text goes straight into g_err.
__attribute__((format(printf, 2, 3))) inline int failf(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// Workgroups of `per` elements that cover n.
inline unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// 0 when e (default: the pending launch error) is hipSuccess, else -5 with "<what>: <hip's text>".
inline int hip_status(const char* what, hipError_t e = hipGetLastError()) {
    if (e == hipSuccess) return 0;
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -5;
}

// 256-row blocks of the TD loss per net (td_loss_kernel: one loss partial each), as td_launch
// launches them, evx_td_loss_ws_floats sizes them and evx_qmlp_group_plan reports them.
inline int td_blocks(int B) { return (B + 255) / 256; }

// Compute units of the current device (cached per device; 256 if the query fails).
inline int cu_count() {
    static std::atomic<int> ncu[64];
    const int d = cur_device();
    int n = 0;
    if (d >= 0 && d < 64 && (n = ncu[d].load(std::memory_order_relaxed)) > 0) return n;
    if (d < 0 || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n <= 0) n = 256;
    if (d >= 0 && d < 64) ncu[d].store(n, std::memory_order_relaxed);
    return n;
}

}  // namespace evxh
