// kafka_host.cpp -- the Kafka message-set core (flowgger_amd/csrc/fg_kafka.hpp) on the CPU, a wave being 64 fibers, in the order the kernels
// of fg_kafka.hip run it (test infrastructure).
#include "kafka_driver.hpp"

extern "C" uint32_t fgk_overhead() { return fg::kafka::kOverhead; }
extern "C" uint32_t fgk_row_max() { return fg::kafka::kRowMax; }
extern "C" uint32_t fgk_piece() { return fg::kafka::kPiece; }
extern "C" uint64_t fgk_bound(uint64_t nbytes, uint64_t n, uint64_t n_members) { return fg::kafka::bound(nbytes, n, n_members); }
extern "C" uint64_t fgk_messageset(const uint8_t* bytes, uint64_t nbytes, const uint64_t* off, const uint8_t* skip, uint64_t n, uint8_t* set, uint64_t set_cap,
                                   uint64_t* set_off) {
    return fgk::messageset(bytes, nbytes, off, skip, n, set, set_cap, set_off);
}
extern "C" uint64_t fgk_wrap(const uint8_t* z, const uint64_t* z_off, uint64_t n_members, uint8_t* w, uint64_t w_cap, uint64_t* w_off) {
    return fgk::wrap_members(z, z_off, n_members, w, w_cap, w_off);
}
extern "C" void fgk_cuts(const uint64_t* set_off, const uint64_t* member_first, uint64_t n, uint64_t n_members, uint64_t* set_cuts) {
    fgk::cuts(set_off, member_first, n, n_members, set_cuts);
}
