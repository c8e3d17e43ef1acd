// fg_cus.hpp -- the compute units of the device a launch goes to: the one way every launcher and the C ABI ask for them.
#pragma once
#include <hip/hip_runtime.h>

namespace fg {

// Compute units of the CURRENT device (the C ABI's DeviceGuard has selected the ctx's); 0 = no device or a HIP error.  One attribute
// query per call -- a process may drive several devices -- and never hipGetDeviceProperties, which fills a few hundred fields.
inline int device_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
#if defined(__HIPCC__)
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
#else
    // (a host compiler: the host side of the C ABI built against the CPU suite's stand-in runtime, tests/native/fakehip, which
    //  answers the properties call only; the library itself is compiled by hipcc and never takes this branch)
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    cus = prop.multiProcessorCount;
#endif
    return cus < 1 ? 0 : cus;
}

}  // namespace fg
