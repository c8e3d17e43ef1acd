// host_pipeline_fake_capnp.cpp (the fake launchers of host_pipeline_fake.cpp plus a fake FG_CAPNP decode launcher) with a look at the one
// capacity fg_transcode_multi_batch's grow-and-retry depends on, so that a test can size a batch one byte beyond it.  There is no fake
// octet-counted or Cap'n Proto framer and no fake cut: both framings take their host hop, and the cut is computed on the host.  Test
// infrastructure.
#include "host_pipeline_fake_capnp.cpp"

// the bytes the ctx's device output buffer holds (0: none yet)
extern "C" unsigned long long fgf_tout_cap(const fg_ctx* ctx) { return ctx->d_tout_cap; }
