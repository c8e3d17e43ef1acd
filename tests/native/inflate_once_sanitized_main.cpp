// inflate_once_sanitized_main.cpp -- a stand-alone program around inflate_once_host.cpp for a sanitizer build (test infrastructure):
// reads a file of datagrams (u32 length + bytes each), runs fgo_unpack_batch at the given max_inflated with the policy's stage
// capacities and with every capacity forced to each of the further arguments, and prints "OK <datagrams> <packed bytes> <spilled
// under the policy>".  Every buffer is exactly as large as its contract says (the stages are, inside the shim), and every datagram
// also runs alone in an allocation of its own size.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" uint64_t fgo_unpack_batch(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint32_t max_inflated, const uint32_t* w, uint8_t* out,
                                     uint64_t out_cap, uint64_t* out_offsets, uint8_t* drop, uint8_t* status, uint64_t* n_spilled);

int main(int argc, char** argv) {
    if (argc < 3) return 2;
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
    std::vector<uint64_t> out_offsets(n + 1);
    std::vector<uint8_t> drop(n), status(n);
    uint64_t policy_total = 0, policy_spilled = 0;
    for (int a = 2; a < argc; ++a) {  // a == 2: the policy; then each forced capacity
        std::vector<uint32_t> forced(n, a == 2 ? 0u : (uint32_t)std::strtoul(argv[a], nullptr, 10));
        const uint32_t* w = a == 2 ? nullptr : forced.data();
        uint64_t spilled = 0, single_total = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t len = offsets[i + 1] - offsets[i];
            std::vector<uint8_t> one(bytes.begin() + offsets[i], bytes.begin() + offsets[i + 1]);
            const uint64_t offs[2] = {0, len};
            uint64_t oo[2], sp = 0;
            uint8_t d = 0, st = 0;
            const uint64_t need = fgo_unpack_batch(one.data(), offs, 1, max_inflated, w ? w + i : nullptr, nullptr, 0, oo, &d, &st, &sp);
            if (need == ~0ull) return 1;
            std::vector<uint8_t> out(need);
            if (fgo_unpack_batch(one.data(), offs, 1, max_inflated, w ? w + i : nullptr, out.data(), need, oo, &d, &st, &sp) != need) return 1;
            single_total += need;
        }
        const uint64_t total = fgo_unpack_batch(bytes.data(), offsets.data(), n, max_inflated, w, nullptr, 0, out_offsets.data(), drop.data(), status.data(), &spilled);
        if (total == ~0ull) return 1;
        std::vector<uint8_t> out(total);
        const uint64_t again = fgo_unpack_batch(bytes.data(), offsets.data(), n, max_inflated, w, out.data(), total, out_offsets.data(), drop.data(), status.data(), &spilled);
        if (again != total || single_total != total || out_offsets[n] != total) return 1;
        if (a == 2) {
            policy_total = total;
            policy_spilled = spilled;
        } else if (total != policy_total) {
            return 1;  // (the capacity of a stage changes which walk writes a byte, never the bytes)
        }
    }
    std::printf("OK %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)policy_total, (unsigned long long)policy_spilled);
    return 0;
}
