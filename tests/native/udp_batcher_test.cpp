// udp_batcher_test.cpp -- fg::UdpBatcher (flowgger_amd/host/fg_decoder.hpp) as a program (test infrastructure).
//   udp_batcher_test run <file> <max_lines>   datagrams (u32 length, bytes) through a GelfDecoder's batcher: one line per datagram on
//                                             stdout, in arrival order -- "R\t<hostname>\t<bytes of msg>" or the text the reference prints
//   udp_batcher_test fail                     against a library whose fg_udp_decode_batch fails: what a failed flush leaves behind
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <vector>

#include "fg_decoder.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    fg::GelfDecoder dec;
    auto sink = [](fg::Record&& r) { std::cout << "R\t" << r.hostname << "\t" << (r.msg ? r.msg->size() : 0) << "\n"; };
    if (!strcmp(argv[1], "fail")) {
        fg::UdpBatcher ub(dec, sink, std::cout);
        ub.push("abc");
        int threw = 0;
        try { ub.flush(); } catch (const std::runtime_error&) { ++threw; }
        if (threw != 1 || ub.pending() != 1 || ub.pending_bytes() != 3) { printf("after the failed flush: %zu datagrams, %zu bytes\n", ub.pending(), ub.pending_bytes()); return 1; }
        ub.push("defg");
        try { ub.flush(); } catch (const std::runtime_error&) { ++threw; }
        if (threw != 2 || ub.pending() != 2 || ub.pending_bytes() != 7) { printf("after the second: %zu datagrams, %zu bytes\n", ub.pending(), ub.pending_bytes()); return 1; }
        ub.drop();
        if (ub.pending() != 0 || ub.pending_bytes() != 0 || ub.wait_ms() != -1) return 1;
        printf("OK\n");
        return 0;
    }
    if (argc < 4) return 2;
    std::ifstream f(argv[2], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    fg::FlushPolicy pol;
    pol.max_lines = (size_t)atoi(argv[3]);
    pol.max_latency_ms = 100000;  // (only the counts flush here)
    size_t too_large = 0;
    {
        fg::UdpBatcher ub(dec, sink, std::cout, pol, 4096, [&](std::string_view) { ++too_large; });
        for (size_t p = 0; p + 4 <= raw.size();) {
            uint32_t n;
            memcpy(&n, raw.data() + p, 4);
            ub.push(std::string_view(raw.data() + p + 4, n));
            p += 4 + n;
        }
    }  // (the destructor flushes the rest)
    std::cout << "too_large\t" << too_large << "\n";
    return 0;
}
