// mc_owned.h - the owners of what the library takes from the HIP runtime: device buffers, pinned host buffers, streams, events.
// The rule: a resource is a member of one of these types, or lives in the McDevBuf / McEvents of one call; no
// function frees by name, and the eight calls that make and destroy resources are written here and nowhere else in csrc/.
// No HIP include of its own: the includer declares the runtime (mc_hip_common.h; a fake in tests/emul/owned.cpp) and the error
// string g_err.  A failed call leaves "<call>: <hip error>" there, as HIPCK does, and returns -1.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

// how many of each kind are alive in the process (mc_debug_live): counted where one is made and where it is destroyed
enum { MC_LIVE_DEV = 0, MC_LIVE_PIN, MC_LIVE_STREAM, MC_LIVE_EVENT, MC_LIVE_N };
inline std::atomic<int64_t> mc_live[MC_LIVE_N];

static inline int mc_owned_ck(hipError_t e, const char *call)
{
    if (e == hipSuccess) return 0;
    g_err = std::string(call) + ": " + hipGetErrorString(e);
    return -1;
}

// One resource of kind K behind its runtime handle X (a pointer in all four kinds); move-only, empty when null.
template <class X, int K> struct McOwned {
    McOwned() = default;
    McOwned(McOwned &&o) noexcept : x(o.x) { o.x = nullptr; }
    McOwned &operator=(McOwned &&o) noexcept { if (this != &o) { reset(); x = o.x; o.x = nullptr; } return *this; }
    ~McOwned() { reset(); }
    operator X() const { return x; }
    X get() const { return x; }                                    // (where a cast to another pointer type follows)
    void reset()
    {
        if (!x) return;
        if constexpr (K == MC_LIVE_DEV) (void)hipFree(x);
        else if constexpr (K == MC_LIVE_PIN) (void)hipHostFree(x);
        else if constexpr (K == MC_LIVE_STREAM) (void)hipStreamDestroy(x);
        else (void)hipEventDestroy(x);
        x = nullptr; mc_live[K]--;
    }
protected:
    int took(hipError_t e, const char *call)                       // what a creating call left in x (hipMalloc of 0 bytes: nothing)
    {
        if (mc_owned_ck(e, call)) { x = nullptr; return -1; }
        if (x) mc_live[K]++;
        return 0;
    }
    X x = nullptr;
};

// n elements of device memory; alloc frees what it held FIRST, so a pool that is replaced never exists twice
template <class Tp> struct McDev : McOwned<Tp *, MC_LIVE_DEV> {
    int alloc(size_t n) { this->reset(); return this->took(hipMalloc((void **)&this->x, n * sizeof(Tp)), "hipMalloc((void **)p, n * sizeof(Tp))"); }
};
// the same of pinned host memory
template <class Tp> struct McPin : McOwned<Tp *, MC_LIVE_PIN> {
    int alloc(size_t n) { this->reset(); return this->took(hipHostMalloc((void **)&this->x, n * sizeof(Tp), hipHostMallocDefault), "hipHostMalloc((void **)p, n * sizeof(Tp), hipHostMallocDefault)"); }
};
struct McStream : McOwned<hipStream_t, MC_LIVE_STREAM> {
    int create() { reset(); return took(hipStreamCreate(&x), "hipStreamCreate(&st)"); }
};
struct McEvent : McOwned<hipEvent_t, MC_LIVE_EVENT> {
    int create(bool timing = true)
    {
        reset();
        return timing ? took(hipEventCreate(&x), "hipEventCreate(&e)") : took(hipEventCreateWithFlags(&x, hipEventDisableTiming), "hipEventCreateWithFlags(&e, hipEventDisableTiming)");
    }
};

// Scoped owners of what a call makes on the device, so that no return path leaves any of it behind: buffers ...
struct McDevBuf {
    std::vector<void *> p;
    template <class Tp> int get(Tp **x, size_t n)
    {
        if (mc_owned_ck(hipMalloc((void **)x, (n ? n : 1) * sizeof(Tp)), "hipMalloc((void **)x, std::max<size_t>(n, 1) * sizeof(Tp))")) { *x = nullptr; return -1; }
        p.push_back(*x); mc_live[MC_LIVE_DEV]++;
        return 0;
    }
    McDevBuf() = default;
    McDevBuf(const McDevBuf &) = delete;
    ~McDevBuf() { for (void *q : p) { (void)hipFree(q); mc_live[MC_LIVE_DEV]--; } }
};
// ... and events
struct McEvents {
    std::vector<hipEvent_t> e;
    int make(int n)
    {
        for (int k = 0; k < n; k++) { hipEvent_t x; if (hipEventCreate(&x) != hipSuccess) { g_err = "hipEventCreate failed"; return -1; } e.push_back(x); mc_live[MC_LIVE_EVENT]++; }
        return 0;
    }
    hipEvent_t operator[](int k) const { return e[(size_t)k]; }
    McEvents() = default;
    McEvents(const McEvents &) = delete;
    ~McEvents() { for (hipEvent_t x : e) { (void)hipEventDestroy(x); mc_live[MC_LIVE_EVENT]--; } }
};
