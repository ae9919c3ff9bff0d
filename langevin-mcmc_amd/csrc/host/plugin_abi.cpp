// The reference's plugin ABI, evaluate_path_bidir_* (described below, where it begins).  Host logic only: the kernels are in device/plugin.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "../device/kernels.h"
#include "hostutil.h"

using namespace lmcd;
using namespace lmc_host;

// ---- the reference's plugin symbols (pathlibbidir_mala.so): 42 forward + 42 derivative programs.
// A single evaluation is one (tiny) kernel launch; throughput users call lmc_grad_batch.
// Per calling thread: a stream and two host-mapped pinned buffers, created on the first call and kept.  A call copies the caller's
// arrays into the input buffer (a few hundred floats, host memcpy), launches ONE single-wave kernel that reads them over the bus and
// writes the result into the output buffer, and waits for the stream: no allocation, no copy call, no device-wide sync (round 2:
// five hipMalloc + three H2D + hipDeviceSynchronize + two D2H per call, 100-200 us).  Re-entrant like the reference's symbols
// (mutation_mala.h:97-110 calls them from every worker thread with thread-private buffers): nothing is shared between threads.
namespace {
struct PluginSlot {
    int device = -1;
    hipStream_t stream = nullptr;
    float *hostIn = nullptr, *hostOut = nullptr, *devIn = nullptr, *devOut = nullptr, *devStage = nullptr;
    void Ensure() {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        if (stream && dev == device) return;
        Release();
        EnsureDevice(dev);
        device = dev;
        HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        HIP_CHECK(hipHostMalloc((void **)&hostIn, (17 + 38 + 600) * sizeof(float), hipHostMallocMapped));
        HIP_CHECK(hipHostMalloc((void **)&hostOut, (1 + 16 + 256) * sizeof(float), hipHostMallocMapped));
        HIP_CHECK(hipHostGetDevicePointer((void **)&devIn, hostIn, 0));
        HIP_CHECK(hipHostGetDevicePointer((void **)&devOut, hostOut, 0));
        HIP_CHECK(hipMalloc((void **)&devStage, (17 + 38 + 600) * sizeof(float)));
    }
    void Release() {
        if (hostIn) (void)hipHostFree(hostIn);
        if (hostOut) (void)hipHostFree(hostOut);
        if (devStage) (void)hipFree(devStage);
        if (stream) (void)hipStreamDestroy(stream);
        hostIn = hostOut = devIn = devOut = devStage = nullptr, stream = nullptr, device = -1;
    }
    ~PluginSlot() { Release(); }
};
thread_local PluginSlot g_pluginSlot;

// returns false (after printing why) when the evaluation could not run: the outputs are NaN then, the reference's own failure convention
bool PluginCall(int c, int l, const float *primary, const float *scene, const float *vertParams, int mode /* 0 value, 1 gradient, 2 Hessian */) {
    try {
        if (!(c >= 1 && l >= 0 && c + l >= 3 && c + l - 1 <= 8)) throw std::runtime_error("technique (c,l) out of range");
        PluginSlot &P = g_pluginSlot;
        P.Ensure();
        const int L = std::max(c + l - 1, 2), V = 238 + 59 * (c + l - 3);
        memcpy(P.hostIn, primary, (size_t)(2 * L + 1) * sizeof(float));
        memcpy(P.hostIn + 17, scene, 38 * sizeof(float));
        memcpy(P.hostIn + 55, vertParams, (size_t)V * sizeof(float));
        if (mode == 2) LaunchPluginHess(c, l, P.devIn, P.devStage, P.devOut, P.stream);
        else
            LaunchPluginGrad(c, l, P.devIn, P.devOut, mode, P.stream);
        HIP_CHECK(hipStreamSynchronize(P.stream));
        return true;
    } catch (const std::exception &e) {
        LmcSetLastError(e.what());
        fprintf(stderr, "lmc: path program (%d,%d) failed: %s\n", c, l, e.what());
        return false;
    }
}
}  // namespace
static void PluginEval(int c, int l, const float *primary, const float *scene, const float *vertParams, float *logLum, float *grad) {
    const int L = std::max(c + l - 1, 2);
    const bool ok = PluginCall(c, l, primary, scene, vertParams, grad ? 1 : 0);
    const float *o = g_pluginSlot.hostOut;
    if (logLum) logLum[0] = ok ? o[0] : NAN;
    if (grad)
        for (int k = 0; k < 2 * L; k++) grad[k] = ok ? o[1 + k] : NAN;
}
static void PluginEvalHess(int c, int l, const float *primary, const float *scene, const float *vertParams, float *grad, float *hess) {
    const int L = std::max(c + l - 1, 2), dim = 2 * L;
    const bool ok = PluginCall(c, l, primary, scene, vertParams, 2);
    const float *o = g_pluginSlot.hostOut;
    if (grad)
        for (int k = 0; k < dim; k++) grad[k] = ok ? o[1 + k] : NAN;
    if (hess)
        for (int k = 0; k < dim * dim; k++) hess[k] = ok ? o[17 + k] : NAN;
}
extern "C" {
#define LMC_PLUGIN(C, Lg)                                                                                                                          \
    void evaluate_path_bidir_mala_##C##_##Lg##_static(const float *, const float *primary, const float *scene, const float *vp, float *logLum) {   \
        PluginEval(C, Lg, primary, scene, vp, logLum, nullptr);                                                                                    \
    }                                                                                                                                              \
    void evaluate_path_bidir_mala_##C##_##Lg##_static_derv(const float *, const float *primary, const float *scene, const float *vp, float *grad) { \
        PluginEval(C, Lg, primary, scene, vp, nullptr, grad);                                                                                      \
    }                                                                                                                                              \
    /* H2MC library (pathlibbidir.so, chad.cpp:884-895; caller mutation_h2mc.h:74-79): same forward program, derivative with Hessian */          \
    void evaluate_path_bidir_##C##_##Lg##_static(const float *, const float *primary, const float *scene, const float *vp, float *logLum) {        \
        PluginEval(C, Lg, primary, scene, vp, logLum, nullptr);                                                                                    \
    }                                                                                                                                              \
    void evaluate_path_bidir_##C##_##Lg##_static_derv(const float *, const float *primary, const float *scene, const float *vp, float *grad, float *hess) { \
        PluginEvalHess(C, Lg, primary, scene, vp, grad, hess);                                                                                     \
    }
// (c,l) with 1<=c<=9, 0<=l<=8, 3<=c+l<=9 (path.cpp:3955-3959)
LMC_PLUGIN(1, 2) LMC_PLUGIN(1, 3) LMC_PLUGIN(1, 4) LMC_PLUGIN(1, 5) LMC_PLUGIN(1, 6) LMC_PLUGIN(1, 7) LMC_PLUGIN(1, 8)
LMC_PLUGIN(2, 1) LMC_PLUGIN(2, 2) LMC_PLUGIN(2, 3) LMC_PLUGIN(2, 4) LMC_PLUGIN(2, 5) LMC_PLUGIN(2, 6) LMC_PLUGIN(2, 7)
LMC_PLUGIN(3, 0) LMC_PLUGIN(3, 1) LMC_PLUGIN(3, 2) LMC_PLUGIN(3, 3) LMC_PLUGIN(3, 4) LMC_PLUGIN(3, 5) LMC_PLUGIN(3, 6)
LMC_PLUGIN(4, 0) LMC_PLUGIN(4, 1) LMC_PLUGIN(4, 2) LMC_PLUGIN(4, 3) LMC_PLUGIN(4, 4) LMC_PLUGIN(4, 5)
LMC_PLUGIN(5, 0) LMC_PLUGIN(5, 1) LMC_PLUGIN(5, 2) LMC_PLUGIN(5, 3) LMC_PLUGIN(5, 4)
LMC_PLUGIN(6, 0) LMC_PLUGIN(6, 1) LMC_PLUGIN(6, 2) LMC_PLUGIN(6, 3)
LMC_PLUGIN(7, 0) LMC_PLUGIN(7, 1) LMC_PLUGIN(7, 2)
LMC_PLUGIN(8, 0) LMC_PLUGIN(8, 1)
LMC_PLUGIN(9, 0)
}  // extern "C"
