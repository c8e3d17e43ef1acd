// host_stages_san_main.cpp -- the host side of the output stages (flowgger_amd/csrc/fg_capi.cpp and fg_host_pipeline.cpp: the scratch
// layouts carved by fg_ctx.hpp's Carver, the member stage of the transcode entry points, the sized resident calls) in a stand-alone
// program for -fsanitize=address,undefined, on the fake runtime and launchers of host_pipeline_fake_kafka.cpp.  "Device" memory is
// malloc'd there, so a layout whose walk leaves the bytes its size asked for is a heap overflow here.  Driven:
//   - every wire x codec x member policy x deflate mode through the three transcode entries, twice per ctx (cold and warm);
//   - the five sized resident entries at n = 0, 1, 63, 64, 65, 130 (the per-64 sums change shape at a multiple of 64): as a sizing
//     call, into a buffer of exactly the total, and into one a byte short;
//   - a failed runtime call at every call index of one kafka + gzip transcode.
// Exits non-zero on a wrong return code or total.  Nothing here is loaded into Python.  Test infrastructure.
#include <stdio.h>

#include <memory>
#include <string>
#include <vector>

#include "host_pipeline_fake_kafka.cpp"

#include "deflate_dyn_driver.hpp"

// ---- the launchers no fake library has: FG_DEFLATE_DYNAMIC's blocks beside the Kafka launchers, and fg_udp_unpack_device's three
extern "C" int fg_launch_deflate_blocks_dyn(const uint8_t* d_bytes, const uint64_t* d_cuts, const uint64_t* d_blk_first, uint64_t n_members,
                                            uint64_t n_blocks, uint8_t* d_slots, uint64_t slots_cap, uint32_t* d_blk_size, uint32_t* d_blk_crc,
                                            uint32_t* d_ticket, int, hipStream_t s) {
    FAKE_LAUNCH(s);
    if (n_blocks != d_blk_first[n_members] || slots_cap < fg::deflate::slot_bytes(d_cuts[n_members], n_blocks)) return -9;
    *d_ticket = (uint32_t)n_blocks;
    fgd::blocks_dyn(d_bytes, d_cuts, d_blk_first, n_members, d_slots, d_blk_size, d_blk_crc, nullptr);
    return 0;
}
namespace inf = fg::inflate;
extern "C" int fg_launch_udp_count(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint32_t max_inflated, uint32_t* d_sizes,
                                   uint64_t* d_block_sums, uint8_t* d_status, uint8_t* d_drop, hipStream_t s) {
    FAKE_LAUNCH(s);
    uint16_t h[inf::kHalfWords];
    uint8_t b[inf::kLenBytes];
    const inf::Tabs t{h, b, 1u};
    for (uint64_t i = 0; i < n; ++i) {
        d_status[i] = (uint8_t)inf::count_datagram(d_bytes + d_offsets[i], d_offsets[i + 1] - d_offsets[i], max_inflated, t, &d_sizes[i]);
        d_drop[i] = d_status[i] > inf::UDP_GZIP;
        if (i % 64 == 0) d_block_sums[i / 64] = 0;
        d_block_sums[i / 64] += d_sizes[i];
    }
    return 0;
}
extern "C" int fg_launch_udp_write(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out,
                                   uint64_t out_cap, uint8_t* d_status, uint8_t* d_drop, hipStream_t s) {
    FAKE_LAUNCH(s);
    if (d_out_offsets[n] > out_cap) return -9;
    uint16_t h[inf::kHalfWords];
    uint8_t b[inf::kLenBytes];
    const inf::Tabs t{h, b, 1u};
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* p = d_bytes + d_offsets[i];
        const uint64_t len = d_offsets[i + 1] - d_offsets[i], size = d_out_offsets[i + 1] - d_out_offsets[i];
        if (d_status[i] == inf::UDP_RAW) {
            if (size) memcpy(d_out + d_out_offsets[i], p, size);
            continue;
        }
        const uint32_t st = inf::write_datagram(p, len, d_status[i], (uint32_t)size, t, d_out + d_out_offsets[i]);
        if (st != d_status[i]) {
            d_status[i] = (uint8_t)st;
            d_drop[i] = 1;
        }
    }
    return 0;
}
extern "C" int fg_launch_udp_finish(const uint8_t*, const uint64_t*, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out, uint64_t, uint8_t* d_status,
                                    uint8_t* d_drop, hipStream_t s) {
    FAKE_LAUNCH(s);
    for (uint64_t i = 0; i < n; ++i)
        if (!d_drop[i] && fg::utf8::payload_bad(d_out + d_out_offsets[i], (uint32_t)(d_out_offsets[i + 1] - d_out_offsets[i]))) {
            d_status[i] = (uint8_t)inf::UDP_BAD_UTF8;
            d_drop[i] = 1;
        }
    return 0;
}

namespace {
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, g_where.c_str()); \
            return 1;                                                        \
        }                                                                    \
    } while (0)
std::string g_where;

// `count` ASCII records with a few '=' each (the fake decode makes an entry of each, the fake encoder a '#'), rows 3, 17 and 18 empty
// (they fail the fake decode: empty messages inside the members)
std::vector<std::string> records(size_t count) {
    std::vector<std::string> v;
    uint32_t x = 2463534242u;
    for (size_t i = 0; i < count; ++i) {
        std::string r;
        x = x * 1664525u + 1013904223u;
        const uint32_t pairs = 1u + (x >> 28), pad = (x >> 8) % 90u;
        for (uint32_t k = 0; k < pairs; ++k) r += "key" + std::to_string(k) + "=v" + std::to_string((x >> k) & 1023u) + " ";
        r += std::string(pad, (char)('a' + i % 26));
        v.push_back(i == 3 || i == 17 || i == 18 ? std::string() : r);
    }
    return v;
}
// a zlib stream of one stored block (at most 65535 bytes)
std::string zlib_stored(const std::string& r) {
    uint32_t a = 1, b = 0;
    for (unsigned char ch : r) {
        a = (a + ch) % 65521u;
        b = (b + a) % 65521u;
    }
    const uint16_t len = (uint16_t)r.size();
    std::string z = {(char)0x78, (char)0x01, (char)0x01, (char)(len & 0xFF), (char)(len >> 8), (char)(~len & 0xFF), (char)((~len >> 8) & 0xFF)};
    z += r;
    for (int sh = 24; sh >= 0; sh -= 8) z.push_back((char)(((b << 16) | a) >> sh));  // Adler-32, big-endian
    return z;
}
// the pieces back to back in an allocation that ends with the last byte, and their n + 1 bounds
struct Packed {
    std::unique_ptr<uint8_t[]> bytes;
    std::vector<uint64_t> off{0};
    explicit Packed(const std::vector<std::string>& pieces, const char* sep = "") {
        std::string all;
        for (const std::string& p : pieces) {
            all += p + sep;
            off.push_back(all.size());
        }
        bytes.reset(new uint8_t[all.size() ? all.size() : 1]);
        memcpy(bytes.get(), all.data(), all.size());
    }
    uint64_t size() const { return off.back(); }
};

fg_encode_cfg gelf_lines() {
    fg_encode_cfg e{};
    e.encoder = FG_ENC_GELF;
    e.merger = FG_MERGE_LINE;
    return e;
}
int run_entry(fg_ctx* ctx, int entry, const std::vector<std::string>& recs) {
    const fg_encode_cfg e = gelf_lines();
    if (entry == 0) {
        const Packed p(recs);
        fg_transcoded out;
        return fg_transcode_batch(ctx, FG_RFC5424, FG_FRAME_NONE, &e, p.bytes.get(), p.size(), p.off.data(), recs.size(), 1, &out);
    }
    if (entry == 1) {  // three connections, every third record each
        std::vector<std::string> segs(3);
        for (size_t i = 0; i < recs.size(); ++i) segs[i % 3] += recs[i] + "\n";
        const Packed p(segs);
        fg_transcoded_multi out;
        return fg_transcode_multi_batch(ctx, FG_RFC5424, FG_FRAME_LINE, &e, p.bytes.get(), p.size(), p.off.data(), nullptr, 3, &out);
    }
    std::vector<std::string> grams;
    for (size_t i = 0; i < recs.size(); ++i) grams.push_back(i % 2 && !recs[i].empty() ? zlib_stored(recs[i]) : recs[i]);
    const Packed p(grams);
    fg_transcoded out;
    const uint8_t* ust = nullptr;
    return fg_udp_transcode_batch(ctx, FG_RFC5424, &e, p.bytes.get(), p.size(), p.off.data(), grams.size(), 0, &out, &ust);
}
int configure(fg_ctx* ctx, int wire, int codec, int policy, int mode) {
    const fg_compress_cfg cc{codec ? FG_COMP_GZIP : FG_COMP_NONE, policy ? 0u : 1u, policy ? 4096u : 0u};
    CHECK(fg_set_output_compression(ctx, &cc) == FG_OK && fg_set_output_wire(ctx, wire ? FG_WIRE_KAFKA_V0 : FG_WIRE_RAW) == FG_OK);
    CHECK(fg_set_deflate_mode(ctx, mode ? FG_DEFLATE_DYNAMIC : FG_DEFLATE_FIXED) == FG_OK);
    return 0;
}

int transcode_grid(unsigned long long* cells) {
    const std::vector<std::string> recs = records(300);
    for (int entry = 0; entry < 3; ++entry)
        for (int wire = 0; wire < 2; ++wire)
            for (int codec = 0; codec < 2; ++codec)
                for (int policy = 0; policy < 2; ++policy)
                    for (int mode = 0; mode < 2; ++mode) {
                        g_where = "entry " + std::to_string(entry) + " wire " + std::to_string(wire) + " codec " + std::to_string(codec) + " policy " +
                                  std::to_string(policy) + " mode " + std::to_string(mode);
                        fg_ctx* ctx = nullptr;
                        CHECK(fg_create(0, nullptr, &ctx) == FG_OK);
                        if (configure(ctx, wire, codec, policy, mode)) return 1;
                        for (int pass = 0; pass < 2; ++pass) {
                            CHECK(run_entry(ctx, entry, recs) == FG_OK && fakehip::in_flight() == 0);
                            fg_compressed z;
                            CHECK(fg_last_compressed(ctx, &z) == FG_OK);
                            CHECK((z.n_members != 0) == (wire || codec) && (!z.n_members || (z.z_offsets[0] == 0 && z.z_offsets[z.n_members] == z.z_bytes)));
                        }
                        fg_destroy(ctx);
                        ++*cells;
                    }
    return 0;
}

// One sized entry: call(out, cap, &total).  has_sizing: a NULL buffer is the sizing call (else an argument error).
template <class Call>
int sized(bool has_sizing, uint64_t* total_out, Call&& call) {
    uint64_t total = ~0ull;
    const int rc = call(nullptr, 0, &total);
    CHECK(rc == (has_sizing ? FG_OK : FG_ERR_ARG));
    if (!has_sizing) {  // (the total from a buffer that surely holds it)
        std::unique_ptr<uint8_t[]> big(new uint8_t[1 << 20]);
        CHECK(call(big.get(), 1 << 20, &total) == FG_OK);
    }
    CHECK(total < (1u << 20));
    std::unique_ptr<uint8_t[]> exact(new uint8_t[total ? total : 1]);  // (the allocation ends with the last byte)
    uint64_t again = ~0ull;
    CHECK(call(exact.get(), total, &again) == FG_OK && again == total && fakehip::in_flight() == 0);
    if (total) {
        std::unique_ptr<uint8_t[]> small(new uint8_t[total - 1 ? total - 1 : 1]);
        CHECK(call(small.get(), total - 1, &again) == FG_ERR_ENT_OVERFLOW && again == total && fakehip::in_flight() == 0);
    }
    *total_out = total;
    return 0;
}

int resident_entries(unsigned long long* calls) {
    fg_ctx* ctx = nullptr;
    CHECK(fg_create(0, nullptr, &ctx) == FG_OK);
    for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 130ull}) {
        const std::vector<std::string> recs = records(n);
        std::vector<std::string> grams;
        for (size_t i = 0; i < recs.size(); ++i) grams.push_back(i % 2 && !recs[i].empty() ? zlib_stored(recs[i]) : recs[i]);
        const Packed g(grams), v(recs);
        // (every list exactly as long as the call may write it)
        std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1]), zoff(new uint64_t[n + 1]), woff(new uint64_t[n + 1]);
        std::unique_ptr<uint8_t[]> drop(new uint8_t[n ? n : 1]), st(new uint8_t[n ? n : 1]), skip(new uint8_t[n ? n : 1]);
        for (uint64_t i = 0; i < n; ++i) skip[i] = i % 7 == 5;
        uint64_t total = 0;
        g_where = "fg_udp_unpack_device n " + std::to_string(n);
        if (sized(true, &total, [&](uint8_t* out, uint64_t cap, uint64_t* t) {
                return fg_udp_unpack_device(ctx, g.bytes.get(), g.size(), g.off.data(), n, 0, out, cap, off.get(), drop.get(), st.get(), t, FG_STREAM_OWN);
            }))
            return 1;
        CHECK(total == v.size());
        g_where = "fg_udp_unpack_once_device n " + std::to_string(n);
        if (sized(false, &total, [&](uint8_t* out, uint64_t cap, uint64_t* t) {
                const int rc = fg_udp_unpack_once_device(ctx, g.bytes.get(), g.size(), g.off.data(), n, 0, out, cap, off.get(), drop.get(), st.get(), t,
                                                         FG_STREAM_OWN);
                if (rc == FG_OK && n) {  // (the one entry that returns with its pack queued)
                    if (fakehip::in_flight() == 0 || hipStreamSynchronize(ctx->stream) != hipSuccess) return -100;
                }
                return rc;
            }))
            return 1;
        CHECK(total == v.size());
        for (int mode = 0; mode < 2; ++mode) {
            g_where = "fg_kafka_messageset_device n " + std::to_string(n);
            uint64_t set_bytes = 0;
            if (sized(true, &set_bytes, [&](uint8_t* out, uint64_t cap, uint64_t* t) {
                    return fg_kafka_messageset_device(ctx, v.bytes.get(), v.size(), v.off.data(), skip.get(), n, out, cap, off.get(), t, FG_STREAM_OWN);
                }))
                return 1;
            std::unique_ptr<uint8_t[]> set(new uint8_t[set_bytes ? set_bytes : 1]);
            CHECK(fg_kafka_messageset_device(ctx, v.bytes.get(), v.size(), v.off.data(), skip.get(), n, set.get(), set_bytes, off.get(), &total, FG_STREAM_OWN) == FG_OK);
            g_where = "fg_deflate_device n " + std::to_string(n) + " mode " + std::to_string(mode);
            CHECK(fg_set_deflate_mode(ctx, mode ? FG_DEFLATE_DYNAMIC : FG_DEFLATE_FIXED) == FG_OK);
            uint64_t z_bytes = 0;  // (a member per message of the set)
            if (sized(true, &z_bytes, [&](uint8_t* out, uint64_t cap, uint64_t* t) {
                    return fg_deflate_device(ctx, set.get(), set_bytes, off.get(), n, out, cap, zoff.get(), t, FG_STREAM_OWN);
                }))
                return 1;
            std::unique_ptr<uint8_t[]> z(new uint8_t[z_bytes ? z_bytes : 1]);
            CHECK(fg_deflate_device(ctx, set.get(), set_bytes, off.get(), n, z.get(), z_bytes, zoff.get(), &total, FG_STREAM_OWN) == FG_OK);
            g_where = "fg_kafka_wrap_device n " + std::to_string(n) + " mode " + std::to_string(mode);
            if (sized(true, &total, [&](uint8_t* out, uint64_t cap, uint64_t* t) {
                    return fg_kafka_wrap_device(ctx, z.get(), zoff.get(), n, out, cap, woff.get(), t, FG_STREAM_OWN);
                }))
                return 1;
            CHECK(n == 0 || total > z_bytes);
        }
        *calls += 8;
    }
    fg_destroy(ctx);
    return 0;
}

int fault_at_every_call(unsigned long long* faults) {
    g_where = "fault injection";
    const std::vector<std::string> recs = records(120);
    fg_ctx* ctx = nullptr;
    CHECK(fg_create(0, nullptr, &ctx) == FG_OK);
    if (configure(ctx, 1, 1, 1, 0)) return 1;
    CHECK(run_entry(ctx, 0, recs) == FG_OK);  // (the ctx's buffers exist from here on)
    const unsigned long long c0 = fakehip::calls();
    CHECK(run_entry(ctx, 0, recs) == FG_OK);
    const unsigned long long calls = fakehip::calls() - c0;
    CHECK(calls >= 25);
    for (unsigned long long i = 1; i <= calls; ++i) {
        g_where = "fault injection at call " + std::to_string(i);
        fakehip::fail_call_after() = (long long)i;
        const int rc = run_entry(ctx, 0, recs);
        fakehip::fail_call_after() = -1;
        CHECK(rc == FG_ERR_HIP && fakehip::in_flight() == 0);
        CHECK(run_entry(ctx, 0, recs) == FG_OK && fakehip::in_flight() == 0);
        ++*faults;
    }
    fg_destroy(ctx);
    return 0;
}
}  // namespace

int main() {
    fgd::lane_stack() = fgk::lane_stack() = 32u << 10;  // (as deflate_san_main.cpp: the cores keep a few dozen words on a lane's stack)
    unsigned long long cells = 0, calls = 0, faults = 0;
    if (transcode_grid(&cells) || resident_entries(&calls) || fault_at_every_call(&faults)) return 1;
    printf("ok %llu cells %llu resident %llu faults\n", cells, calls, faults);
    return 0;
}
