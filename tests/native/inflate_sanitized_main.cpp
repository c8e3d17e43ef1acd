// inflate_sanitized_main.cpp -- a stand-alone program around inflate_host.cpp for a sanitizer build (test infrastructure):
// reads a file of datagrams (u32 length + bytes each), runs fgi_unpack_batch at the given max_inflated as the tests do -- the sizing
// call, then the call that writes -- and prints "OK <datagrams> <packed bytes>".  Every buffer is exactly as large as its contract
// says, so that a byte read or written past one is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" uint64_t fgi_unpack_batch(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint32_t max_inflated, uint8_t* out, uint64_t out_cap,
                                     uint64_t* out_offsets, uint8_t* drop, uint8_t* status);

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + k);
    std::fclose(f);
    const uint32_t max_inflated = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offsets{0};
    for (size_t at = 0; at < file.size();) {
        if (file.size() - at < 4) return 2;
        uint32_t len;
        std::memcpy(&len, file.data() + at, 4);
        at += 4;
        if (file.size() - at < len) return 2;
        bytes.insert(bytes.end(), file.begin() + at, file.begin() + at + len);
        offsets.push_back(bytes.size());
        at += len;
    }
    const uint64_t n = offsets.size() - 1;
    // the datagrams one by one as well, each in an allocation of its own size: a read past a datagram's end cannot land in its neighbour
    uint64_t single_total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        std::vector<uint8_t> one(bytes.begin() + offsets[i], bytes.begin() + offsets[i + 1]);
        const uint64_t offs[2] = {0, len};
        uint64_t oo[2];
        uint8_t drop = 0, st = 0;
        const uint64_t need = fgi_unpack_batch(one.data(), offs, 1, max_inflated, nullptr, 0, oo, &drop, &st);
        std::vector<uint8_t> out(need);
        if (fgi_unpack_batch(one.data(), offs, 1, max_inflated, out.data(), need, oo, &drop, &st) != need) return 1;
        single_total += need;
    }
    std::vector<uint64_t> out_offsets(n + 1);
    std::vector<uint8_t> drop(n), status(n);
    const uint64_t total = fgi_unpack_batch(bytes.data(), offsets.data(), n, max_inflated, nullptr, 0, out_offsets.data(), drop.data(), status.data());
    std::vector<uint8_t> out(total);
    const uint64_t again = fgi_unpack_batch(bytes.data(), offsets.data(), n, max_inflated, out.data(), total, out_offsets.data(), drop.data(), status.data());
    if (again != total || single_total != total || out_offsets[n] != total) return 1;
    std::printf("OK %llu %llu\n", (unsigned long long)n, (unsigned long long)total);
    return 0;
}
