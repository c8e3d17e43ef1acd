// Host build of the Cap'n Proto emitter (flowgger_amd/csrc/fg_emit.hpp CapnpEmitter + its configuration, fg_enc_cfg.hpp) exactly as
// the kernels run it, driven from a canonical Record.  emit_host.cpp's helpers (reader, escaping of the synthetic source text) are
// reused; the one-row table is laid out here the same way.  Test infrastructure only -- the product has no CPU path.
#include "emit_host.cpp"

// As fge_encode_canonical for FG_ENC_CAPNP: the count pass, then the write pass at all sixteen start alignments inside a guarded
// buffer.  Returns the output length (written when <= cap); -1 bad record / configuration, -2 key without '_', -3 count and write
// passes disagree, -4 a byte outside the message changed, -5 the alignments disagree.
extern "C" int64_t fgc_encode_canonical(int merger, int src_fmt, uint64_t seed, const uint8_t* canonical, uint64_t len,
                                        const char* const* extra_keys, const char* const* extra_vals, uint32_t n_extra, double now_ts,
                                        uint8_t* out, uint64_t cap, uint32_t* status) {
    rng_state = seed * 2654435761u + 12345u;
    Cur c{canonical, len};
    if (c.u8() != 0) return -1;
    const bool ts_now = c.u8() != 0;
    uint64_t tsb = c.u64();
    const uint32_t fac = c.u8(), sev = c.u8();
    std::string line(16, 'x');
    uint32_t flags = ts_now ? FG_F_TS_NOW : 0;
    fg_span cols[6];
    const uint32_t escbit[6] = {FG_F_HOST_ESC, 0, 0, 0, FG_F_MSG_ESC, FG_F_FULLMSG_ESC};
    for (int k = 0; k < 6; ++k) {
        if (!c.u8()) { cols[k] = fg_span{0, FG_NONE}; continue; }
        std::string s = c.str();
        bool esc = false;
        if (src_fmt == FG_GELF && escbit[k]) s = json_escape_src(s, &esc);
        if (src_fmt == FG_RFC3164 && k == fg::S_MSG) {  // the decoder's source text: runs of whitespace where the Record has one space
            std::string o;
            for (char ch : s) {
                o.push_back(ch);
                if (ch == ' ' && (rnd() & 1)) { o += (rnd() & 1) ? " \t" : "  "; esc = true; }
            }
            if (rnd() & 1) { o = " " + o + "\t "; esc = true; }
            s = o;
            if (esc) flags |= FG_F_MSG_JOIN;
            esc = false;
        }
        if (esc) flags |= escbit[k];
        line += "|";
        cols[k] = fg_span{(uint32_t)line.size(), (uint32_t)s.size()};
        line += s;
    }
    std::vector<fg_span> en;
    std::vector<uint64_t> ev;
    std::vector<uint8_t> et, ef;
    if (c.u8()) {
        const uint32_t nsd = c.u32();
        for (uint32_t a = 0; a < nsd; ++a) {
            const bool has_id = c.u8() != 0;
            std::string id = has_id ? c.str() : "";
            if (src_fmt == FG_RFC5424) {
                line += "[";
                en.push_back(fg_span{(uint32_t)line.size(), (uint32_t)id.size()});
                line += id;
                ev.push_back(0);
                et.push_back(FG_T_SDID);
                ef.push_back(0);
            }
            const uint32_t np = c.u32();
            for (uint32_t b = 0; b < np; ++b) {
                std::string key = c.str();
                const uint32_t ty = c.u8();
                uint8_t fl = 0;
                if (key.empty() || key[0] != '_') return -2;
                std::string name = src_fmt == FG_GELF ? key : key.substr(1);
                bool esc = false;
                if (src_fmt == FG_GELF) name = json_escape_src(name, &esc);
                if (esc) fl |= FG_EF_NAME_ESC;
                line += " ";
                en.push_back(fg_span{(uint32_t)line.size(), (uint32_t)name.size()});
                line += name;
                uint64_t v = 0;
                if (ty == FG_T_STRING) {
                    std::string s = c.str();
                    bool vesc = false;
                    if (src_fmt == FG_RFC5424) s = sd_escape(s, &vesc);
                    else if (src_fmt == FG_GELF) s = json_escape_src(s, &vesc);
                    if (vesc) fl |= FG_EF_VAL_ESC;
                    line += "=";
                    v = (uint64_t)line.size() | ((uint64_t)s.size() << 32);
                    line += s;
                } else if (ty == FG_T_BOOL) {
                    v = c.u8();
                } else if (ty != FG_T_NULL) {
                    v = c.u64();
                }
                ev.push_back(v);
                et.push_back((uint8_t)ty);
                ef.push_back(fl);
            }
        }
    }
    if (!c.ok || c.i != len) return -1;
    line += "  tail";
    line.resize(line.size() + 16, 'y');  // (the kernels' readers may fetch a whole 16-byte chunk: the staged tile has it)
    const uint64_t li = 3;
    std::vector<uint32_t> meta(5, 0xFFFFFFFFu), ent_first(5, 0), ent_count(5, 0);
    std::vector<double> ts(5, 0.0);
    std::vector<fg_span> span[6];
    for (int k = 0; k < 6; ++k) {
        span[k].assign(5, fg_span{0, FG_NONE});
        span[k][li] = cols[k];
    }
    meta[li] = 0u | fac << 8 | sev << 16 | flags << 24;
    memcpy(&ts[li], &tsb, 8);
    const uint32_t base = 7;
    std::vector<fg_span> ent_name(base + en.size() + 1, fg_span{0, 0});
    std::vector<uint64_t> ent_val(base + en.size() + 1, 0);
    std::vector<uint8_t> ent_type(base + en.size() + 1, 0), ent_flags(base + en.size() + 1, 0);
    for (size_t k = 0; k < en.size(); ++k) {
        ent_name[base + k] = en[k];
        ent_val[base + k] = ev[k];
        ent_type[base + k] = et[k];
        ent_flags[base + k] = ef[k];
    }
    ent_first[li] = base;
    ent_count[li] = (uint32_t)en.size();
    fg::DevTables t{};
    t.n = 5;
    t.ent_cap = ent_name.size();
    t.meta = meta.data();
    t.ts = ts.data();
    for (int k = 0; k < 6; ++k) t.span[k] = span[k].data();
    t.ent_first = ent_first.data();
    t.ent_count = ent_count.data();
    t.ent_name = ent_name.data();
    t.ent_val = ent_val.data();
    t.ent_type = ent_type.data();
    t.ent_flags = ent_flags.data();

    fg_encode_cfg ec{};
    ec.encoder = FG_ENC_CAPNP;
    ec.merger = (fg_merger)merger;
    ec.n_extra = n_extra;
    ec.extra_keys = extra_keys;
    ec.extra_values = extra_vals;
    ec.prepend = "ignored by this encoder";
    ec.now_ts = now_ts;
    const std::string suffix[4];
    const bool has_suffix[4] = {false, false, false, false};
    fg::EncCfgHost h;
    if (!fg::build_enc_cfg((fg_format)src_fmt, &ec, suffix, has_suffix, &h)) return -1;
    h.cfg.blob = h.blob.data();
    h.cfg.keys = h.keys.data();

    uint64_t keys64[1];
    uint8_t slot_ent[1], order[1];
    HostReader rd{(const uint8_t*)line.data()};
    uint32_t st = 0, size = 0;
    std::vector<uint8_t> res;
    for (uint32_t al = 0; al < 16; ++al) {
        uint32_t plain = 0;
        size = fg::emit::row_size<FG_ENC_CAPNP>(h.cfg, rd, t, li, meta[li], keys64, slot_ent, order, &st, nullptr, &plain);
        std::vector<uint8_t> buf((size_t)size + 96, 0xA5);
        uint8_t* start = buf.data() + 32;
        start += (al - ((uintptr_t)start & 15u)) & 15u;
        fg::emit::PackSink sink(start);
        fg::emit::RowRegs pre;  // odd alignments: the row in registers, as the write kernel hands it over
        pre.load(t, li);
        pre.plain = plain;
        fg::emit::row_write<FG_ENC_CAPNP>(sink, size, h.cfg, rd, t, li, meta[li], keys64, slot_ent, order, (al & 1u) ? &pre : nullptr);
        for (uint8_t* q = buf.data(); q < buf.data() + buf.size(); ++q)
            if ((q < start || q >= start + size) && *q != 0xA5) return -4;
        if (size && sink.p != start + size) return -3;
        std::vector<uint8_t> got(start, start + size);
        if (al && got != res) return -5;
        res = got;
    }
    if (status) *status = st;
    if (out && res.size() <= cap) memcpy(out, res.data(), res.size());
    return (int64_t)res.size();
}
