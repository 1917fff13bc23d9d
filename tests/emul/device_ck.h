// tests/emul/device_ck.h - what the device harnesses (device_order.hip, device_coverage.hip, device_ties.hip) share beside order_io.h:
// every HIP call checked - an error is printed and ends the program with status 3 at once - a device array with padding behind it, and a
// stream and an event for the harnesses that hand the library's launch functions side streams (device_order.hip).
// Included behind the HIP runtime (mc_hip_common.h).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(call)                                                                                                            \
    do {                                                                                                                    \
        hipError_t e_ = (call);                                                                                             \
        if (e_ != hipSuccess) { fprintf(stderr, "HIP error: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); fflush(stderr); exit(3); } \
    } while (0)
#define CK_LAUNCH() do { CK(hipGetLastError()); CK(hipDeviceSynchronize()); } while (0)

// a stream and an event (no timing) of the harness' own, destroyed with the object
struct Stream { hipStream_t s = nullptr; Stream() { CK(hipStreamCreate(&s)); } Stream(const Stream &) = delete; ~Stream() { (void)hipStreamDestroy(s); } operator hipStream_t() const { return s; } };
struct Event { hipEvent_t e = nullptr; Event() { CK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); } Event(const Event &) = delete; ~Event() { (void)hipEventDestroy(e); } operator hipEvent_t() const { return e; } };
// a launch function of csrc/mc_stages.h: its -1 (g_err says which call) ends the program like any other HIP error, then CK_LAUNCH
#define CK_STAGE(call) do { if ((call) != 0) { fprintf(stderr, "HIP error: %s: %s (line %d)\n", #call, g_err.c_str(), __LINE__); fflush(stderr); exit(3); } CK_LAUNCH(); } while (0)

// a device array: uploaded or filled with one byte, read back whole, freed with the object.  16 elements of padding lie behind it,
// filled with the same byte (zeros behind an uploaded array): pad() reads them back, and a test asserts that no kernel wrote there
template <class T> struct Dev {
    T *p = nullptr; size_t n = 0;
    Dev(size_t count, int fill = 0) : n(count) { CK(hipMalloc((void **)&p, (n + 16) * sizeof(T))); CK(hipMemset(p, fill, (n + 16) * sizeof(T))); }
    Dev(const T *h, size_t count) : Dev(count) { if (n) CK(hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice)); }
    Dev(const Dev &) = delete;
    ~Dev() { (void)hipFree(p); }
    std::vector<T> host() const { std::vector<T> h(n); if (n) CK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost)); return h; }
    std::vector<T> pad() const { std::vector<T> h(16); CK(hipMemcpy(h.data(), p + n, 16 * sizeof(T), hipMemcpyDeviceToHost)); return h; }
    operator T *() const { return p; }
};
