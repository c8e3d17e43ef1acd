// Host build of flowgger_amd/csrc/fg_capnp_parse.hpp (the per-message Cap'n Proto decode the kernel runs): fills table rows and
// entries for a packed batch so that the product's own fg_tables_serialize can turn them into canonical Records for the
// comparison with the Python model of the reader (tests/capnp_read_model.py).  Test infrastructure only -- the product has no
// CPU decode path.
//
// Every message is parsed out of an EXACT-SIZE private heap copy: with -fsanitize=address (the executable form, -DFGC_MAIN:
// `capnp_in_host_asan <file>`, file = u64 n, u64 offsets[n + 1], the packed bytes) a read outside [offsets[i], offsets[i + 1])
// aborts the run.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/fg_hip.h"
#include "../../flowgger_amd/csrc/fg_capnp_parse.hpp"

namespace {
struct HostWords {
    const uint8_t* p;
    uint64_t word(uint32_t w) const {
        uint64_t v;
        memcpy(&v, p + 8u * (size_t)w, 8);
        return v;
    }
};
struct HostSink {
    fg_tables* t;
    uint32_t first;
    void put(uint32_t k, fg_span name, uint64_t val, uint32_t type, uint32_t flags) {
        t->ent_name[first + k] = name;
        t->ent_val[first + k] = val;
        t->ent_type[first + k] = (uint8_t)type;
        t->ent_flags[first + k] = (uint8_t)flags;
    }
};
}  // namespace

// skipped[i] (may be null) receives the pairs + extras of message i the reference `continue`s over
extern "C" int fgc_decode_batch(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, fg_tables* t, uint32_t* skipped) {
    uint64_t used = 0;
    const fg_span none{0u, FG_NONE};
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        std::vector<uint8_t> copy(bytes + offsets[i], bytes + offsets[i] + (len & ~7ull));
        HostWords rd{copy.data()};
        fg::capnp::Row r;
        fg::capnp::Msg m;
        if (offsets[i] & 7u) r.status = fg::capnp::ST_NO_ROOT;
        else fg::capnp::parse_message(rd, len, r, m);
        if (r.status != fg::capnp::ST_OK) r.n_ent = 0;
        if (skipped) skipped[i] = r.status == fg::capnp::ST_OK ? (r.pairs.ok ? r.pairs.count : 0u) + (r.extra.ok ? r.extra.count : 0u) + (r.sd ? 1u : 0u) - r.n_ent : 0u;
        uint32_t first = 0;
        if (r.n_ent) {
            if (used + r.n_ent > t->ent_cap) {
                r.status = FG_ST_OVERFLOW;
                r.n_ent = 0;
            } else {
                first = (uint32_t)used;
                used += r.n_ent;
                HostSink sink{t, first};
                fg::capnp::emit_entries(rd, m, r, sink);
            }
        }
        const bool ok = r.status == fg::capnp::ST_OK;
        t->meta[i] = r.status | ((ok ? r.fac : 0xFFu) << 8) | ((ok ? r.sev : 0xFFu) << 16);
        double ts = 0.0;
        if (ok) memcpy(&ts, &r.ts_bits, 8);
        t->ts[i] = ts;
        fg_span* cols[6] = {t->hostname, t->appname, t->procid, t->msgid, t->msg, t->full_msg};
        for (int k = 0; k < 6; ++k) cols[k][i] = ok ? r.sp[k] : none;
        t->ent_first[i] = first;
        t->ent_count[i] = r.n_ent;
    }
    if (t->ent_used) *t->ent_used = used;
    return 0;
}

#if defined(FGC_MAIN)
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n = 0;
    if (fread(&n, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> offs(n + 1);
    if (fread(offs.data(), 8, n + 1, f) != n + 1) return 2;
    std::vector<uint8_t> bytes(offs[n]);
    if (offs[n] && fread(bytes.data(), 1, offs[n], f) != offs[n]) return 2;
    fclose(f);
    const uint64_t cap = 1u << 16;
    std::vector<uint32_t> meta(n), first(n), count(n);
    std::vector<double> ts(n);
    std::vector<fg_span> sp[6], en(cap);
    for (auto& v : sp) v.resize(n);
    std::vector<uint64_t> ev(cap);
    std::vector<uint8_t> et(cap), ef(cap);
    uint64_t used = 0;
    fg_tables t{n, cap, meta.data(), ts.data(), sp[0].data(), sp[1].data(), sp[2].data(), sp[3].data(), sp[4].data(), sp[5].data(),
                first.data(), count.data(), en.data(), ev.data(), et.data(), ef.data(), &used};
    fgc_decode_batch(bytes.data(), offs.data(), n, &t, nullptr);
    uint64_t ok = 0;
    for (uint64_t i = 0; i < n; ++i) ok += (meta[i] & 0xFFu) == 0u;
    printf("%llu messages, %llu ok, %llu entries\n", (unsigned long long)n, (unsigned long long)ok, (unsigned long long)used);
    return 0;
}
#endif
