// host_pipeline_fake.cpp plus a fake FG_CAPNP decode launcher (the same deterministic nonsense, one row per message, flagged rows
// skipped), so that fg_frame_decode_capnp_multi_batch runs its bookkeeping on the CPU.  There is no fake framer: the device entry
// answers FG_ERR_UNSUPPORTED and the call walks the segments on the host.  Test infrastructure.
#include "host_pipeline_fake.cpp"

extern "C" int fg_launch_capnp(const uint8_t* b, const uint64_t* o, uint64_t n, const fg::DevTables* t, uint64_t, hipStream_t s, const uint8_t* bad,
                               const fg_launch_opts*, fg::TicketSlot*) {
    FAKE_LAUNCH(s);
    return fake_decode(b, o, n, t, FG_FRAME_NONE, bad);
}
