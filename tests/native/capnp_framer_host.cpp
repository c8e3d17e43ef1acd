// Host build of CapnpFramer (flowgger_amd/host/fg_decoder.hpp) for tests/test_capnp_framer_cpu.py.  Test infrastructure only.
#include "../../flowgger_amd/host/fg_decoder.hpp"

extern "C" int fgc_frame(const uint8_t* buf, uint64_t n, uint64_t* offsets, uint64_t cap, uint64_t* count, uint64_t* consumed) {
    std::vector<uint64_t> offs;
    const int st = (int)fg::CapnpFramer::frame(buf, n, &offs, consumed);
    *count = offs.size();
    for (uint64_t i = 0; i < offs.size() && i < cap; ++i) offsets[i] = offs[i];
    return st;
}
