// What the host units that talk to HIP share (context.cpp, ckpt.cpp, mcrender.cpp, probes.cpp, plugin_abi.cpp, list_probes.cpp): the error check, the
// try / catch brackets of an ABI function, the owning device array, the device check.  Needs HIP, knows no context (context.h).  The g++-built units
// (mcfilm.cpp, shardplan.cpp) include last_error.h alone.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "last_error.h"

#define HIP_CHECK(x)                                                                                                  \
    do {                                                                                                              \
        hipError_t e_ = (x);                                                                                          \
        if (e_ != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #x); \
    } while (0)

// the brackets of an ABI function's body: an exception becomes the message behind lmc_last_error() and the return value `ret`
#define LMC_TRY try {
#define LMC_CATCH(ret)                \
    }                                 \
    catch (const std::exception &e) { \
        LmcSetLastError(e.what());    \
        return ret;                   \
    }

// everything internal that more than one host unit sees lives in this one namespace
namespace lmc_host {

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { Free(); }
    void Free() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void Alloc(size_t count, bool zero = true) {
        Free();
        n = count;
        if (count == 0) return;
        HIP_CHECK(hipMalloc((void **)&p, count * sizeof(T)));
        if (zero) HIP_CHECK(hipMemset(p, 0, count * sizeof(T)));
    }
    void Upload(const std::vector<T> &v) {
        Alloc(v.size(), false);
        if (!v.empty()) HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    void Upload(const T *v, size_t count) {
        Alloc(count, false);
        if (count) HIP_CHECK(hipMemcpy(p, v, count * sizeof(T), hipMemcpyHostToDevice));
    }
    std::vector<T> Download() const {
        std::vector<T> v(n);
        if (n) HIP_CHECK(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
        return v;
    }
};

void EnsureDevice(int device);  // context.cpp: throws unless `device` is a HIP device of this process, and makes it current

inline double MsSince(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }

}  // namespace lmc_host
