// dev_mem.hpp -- host side only: the one place of libaps_hip.so that allocates and frees GPU memory (DevMem), an event
// pair that cleans up after itself, and the driver the four one-shot entry points share (pde_solve_batch, pdew_solve,
// gil_run_batch, gil_run_large).  Who owns what: DESIGN.md "Who owns GPU memory".  Anonymous namespace, like aps_common.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

namespace {

// Owns every allocation it made: frees them in reverse order, each exactly once, when it goes out of scope (or at
// free_all()).  Memory comes back as the runtime hands it out: zero-filling is the caller's choice, per call.
class DevMem {
    struct Rec { void *p; bool host; };       // host: hipHostMalloc'ed (its device address is not a second allocation)
    std::vector<Rec> recs;
    static void free_one(const Rec &r) { (void)(r.host ? hipHostFree(r.p) : hipFree(r.p)); }
    template <typename T> hipError_t keep(hipError_t e, void *q, bool host, T **out) {
        if (e != hipSuccess) return e;
        recs.push_back({q, host});
        *out = static_cast<T *>(q);
        return hipSuccess;
    }

public:
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() { free_all(); }
    void free_all() { for (; !recs.empty(); recs.pop_back()) free_one(recs.back()); }

    // plain device memory, at least one element
    template <typename T> hipError_t alloc(T **out, size_t n) {
        void *q = nullptr;
        return keep(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)), q, false, out);
    }
    // fine-grained device memory (written by a peer while this device polls it); plain where the device has none
    template <typename T> hipError_t alloc_finegrained(T **out, size_t n) {
        void *q = nullptr;
        hipError_t e = hipExtMallocWithFlags(&q, std::max<size_t>(n, 1) * sizeof(T), hipDeviceMallocFinegrained);
        if (e != hipSuccess) { (void)hipGetLastError(); e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)); }
        return keep(e, q, false, out);
    }
    // host memory mapped into the device's address space, with the address the device uses for it
    template <typename T> hipError_t alloc_host_mapped(T **host, T **dev, size_t n) {
        void *q = nullptr;
        if (hipError_t e = keep(hipHostMalloc(&q, std::max<size_t>(n, 1) * sizeof(T), hipHostMallocMapped), q, true, host)) return e;
        return hipHostGetDevicePointer(reinterpret_cast<void **>(dev), *host, 0);
    }
    // frees one allocation ahead of time; null is nothing to free, a pointer this owner did not hand out is reported, not freed
    void release(const void *p) {
        if (!p) return;
        for (size_t i = recs.size(); i-- > 0;)
            if (recs[i].p == p) { free_one(recs[i]); recs.erase(recs.begin() + (long)i); return; }
        std::fprintf(stderr, "DevMem::release: %p is not owned here (programming error); not freed\n", p);
    }
};

// Two events around a timed region: destroys what it created on every path.
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() = default;
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    bool create() { return hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess; }
    void start(hipStream_t s = nullptr) { (void)hipEventRecord(e0, s); }
    void stop(hipStream_t s = nullptr) { (void)hipEventRecord(e1, s); }
    float ms() const { float t = 0.f; (void)hipEventElapsedTime(&t, e0, e1); return t; }
};

// One call of a one-shot entry point `who`: selects the device, owns the call's buffers and events, words the errors
// ("<who>: device upload failed (<field>)") into `err` and returns the caller's own codes; 0 is success everywhere.
struct OneShot {
    const char *who;
    std::string &err;
    bool zero;                                 // zero-fill every buffer (synchronously) before anything else touches it
    int e_nodevice, e_arg, e_hip;
    DevMem mem;
    EventPair ev;

    int fail(int code, const std::string &text) { err = text; return code; }
    int select_device(int ordinal) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(e_nodevice, std::string(who) + ": no HIP device");
        if (ordinal < 0 || ordinal >= ndev) return fail(e_arg, std::string(who) + ": device ordinal out of range");
        if (hipSetDevice(ordinal) != hipSuccess) return fail(e_hip, "hipSetDevice failed");
        return 0;
    }
    template <typename T> int alloc(T **dst, size_t n, const char *field, const char *what = "device allocation failed") {
        if (mem.alloc(dst, n) != hipSuccess) return fail(e_hip, std::string(who) + ": " + what + " (" + field + ")");
        if (zero) (void)hipMemset(const_cast<typename std::remove_const<T>::type *>(*dst), 0, std::max<size_t>(n, 1) * sizeof(T));
        return 0;
    }
    template <typename T> int upload(T **dst, const typename std::remove_const<T>::type *src, size_t n, const char *field) {
        if (int rc = alloc(dst, n, field, "device upload failed")) return rc;
        if (n && hipMemcpy(const_cast<typename std::remove_const<T>::type *>(*dst), src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
            return fail(e_hip, std::string(who) + ": device upload failed (" + field + ")");
        return 0;
    }
    int download(void *host, const void *dev, size_t bytes, const char *field) {
        if (host && hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(e_hip, std::string(who) + ": download failed (" + field + ")");
        return 0;
    }
    int raise_lds_limit(const void *kernel, size_t lds) {
        if (lds > 48 * 1024 && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return fail(e_hip, std::string(who) + ": cannot raise the dynamic LDS limit");
        return 0;
    }
    int create_events() { return ev.create() ? 0 : fail(e_hip, "hipEventCreate failed"); }
    // after ev.stop(): waits for the device; `launch_err` is what the launches themselves reported, `what` prefixes the error
    int finish(hipError_t launch_err, const char *what, double *kernel_ms) {
        const hipError_t serr = hipDeviceSynchronize();
        const hipError_t e = launch_err != hipSuccess ? launch_err : serr;
        if (e != hipSuccess) return fail(e_hip, std::string(what) + ": " + hipGetErrorString(e));
        if (kernel_ms) *kernel_ms = ev.ms();
        return 0;
    }
};

// The four entry points name their argument struct `a` and their OneShot `job`; dst is a member of `a`.
#define UP(dst, src, n) do { if (int rc_ = job.upload(&a.dst, src, n, #dst)) return rc_; } while (0)
#define WORK(dst, n) do { if (int rc_ = job.alloc(&a.dst, n, #dst)) return rc_; } while (0)
#define OUT(dst, host, n) do { if (host) WORK(dst, n); } while (0)
#define DOWN(host, dev, bytes) do { if (int rc_ = job.download(host, a.dev, bytes, #dev)) return rc_; } while (0)

}  // namespace
