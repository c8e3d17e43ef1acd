// fg_table_cols.hpp -- the columns of an fg_tables (include/fg_hip.h) described ONCE, for the host code that sizes, carves, slices,
// shifts, checks or copies a table column by column (fg_capi.cpp, fg_ctx.hpp, fg_host_pipeline.cpp, fg_gather.cpp).  Host-only and
// free of HIP: the kernels keep their own view (fg_tables_view.hpp).  The static_asserts below tie the description to the struct.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>

#include "../../include/fg_hip.h"

namespace fg {

enum ColKind : uint8_t { COL_ROW, COL_ENT, COL_COUNTER };  // one element per row / per entry slot / the single entry counter
struct TableCol {
    uint32_t elem;  // bytes per element
    ColKind kind;
};
// in fg_tables order, which is the order of fg_tables_layout's sizes
constexpr TableCol kTableCols[FG_TABLE_ARRAYS] = {
    {4, COL_ROW}, {8, COL_ROW},                                                          // meta, ts
    {8, COL_ROW}, {8, COL_ROW}, {8, COL_ROW}, {8, COL_ROW}, {8, COL_ROW}, {8, COL_ROW},  // the six spans
    {4, COL_ROW}, {4, COL_ROW},                                                          // ent_first, ent_count
    {8, COL_ENT}, {8, COL_ENT}, {1, COL_ENT}, {1, COL_ENT},                              // ent_name, ent_val, ent_type, ent_flags
    {8, COL_COUNTER},                                                                    // ent_used
};
constexpr int kSpanCol0 = 2, kSpanCols = 6;  // hostname .. full_msg
constexpr int kColEntFirst = 8;              // the one row column a gather rewrites instead of copying

constexpr size_t col_offset(int k) { return offsetof(fg_tables, meta) + (size_t)k * sizeof(void*); }
constexpr uint32_t col_bytes(ColKind kind) {
    uint32_t s = 0;
    for (int k = 0; k < FG_TABLE_ARRAYS; ++k) s += kTableCols[k].kind == kind ? kTableCols[k].elem : 0u;
    return s;
}
constexpr bool spans_ok() {
    for (int k = kSpanCol0; k < kSpanCol0 + kSpanCols; ++k)
        if (kTableCols[k].kind != COL_ROW || kTableCols[k].elem != sizeof(fg_span)) return false;
    return true;
}

#define FG_COL_IS(k, name)                                                                                                           \
    static_assert(offsetof(fg_tables, name) == col_offset(k) && sizeof(*std::declval<fg_tables>().name) == kTableCols[k].elem && \
                      sizeof(std::declval<fg_tables>().name) == sizeof(void*),                                                      \
                  "fg_tables." #name " is not column " #k " of kTableCols")
FG_COL_IS(0, meta);
FG_COL_IS(1, ts);
FG_COL_IS(2, hostname);
FG_COL_IS(3, appname);
FG_COL_IS(4, procid);
FG_COL_IS(5, msgid);
FG_COL_IS(6, msg);
FG_COL_IS(7, full_msg);
FG_COL_IS(8, ent_first);
FG_COL_IS(9, ent_count);
FG_COL_IS(10, ent_name);
FG_COL_IS(11, ent_val);
FG_COL_IS(12, ent_type);
FG_COL_IS(13, ent_flags);
FG_COL_IS(14, ent_used);
#undef FG_COL_IS
static_assert(sizeof(fg_tables) == col_offset(FG_TABLE_ARRAYS), "fg_tables holds a member kTableCols does not describe");
static_assert(col_bytes(COL_ROW) == FG_ROW_BYTES && col_bytes(COL_ENT) == FG_ENT_BYTES && col_bytes(COL_COUNTER) == 8, "column sizes");
static_assert(spans_ok() && kTableCols[kColEntFirst].kind == COL_ROW && kTableCols[kColEntFirst].elem == 4, "named columns");

// column k's pointer, as bytes (a copy of the pointer's representation: no fg_tables member is read through another type)
inline uint8_t* col(const fg_tables& t, int k) {
    uint8_t* p;
    memcpy(&p, reinterpret_cast<const char*>(&t) + col_offset(k), sizeof p);
    return p;
}
inline void set_col(fg_tables* t, int k, const void* p) { memcpy(reinterpret_cast<char*>(t) + col_offset(k), &p, sizeof p); }
inline fg_span* span_col(const fg_tables& t, int j) { return reinterpret_cast<fg_span*>(col(t, kSpanCol0 + j)); }

// byte size of every column for n rows and ent_cap entry slots (what fg_tables_layout answers)
inline void layout(uint64_t n, uint64_t ent_cap, uint64_t sizes[FG_TABLE_ARRAYS]) {
    for (int k = 0; k < FG_TABLE_ARRAYS; ++k) {
        const TableCol& c = kTableCols[k];
        sizes[k] = c.kind == COL_ROW ? n * c.elem : c.kind == COL_ENT ? ent_cap * c.elem : c.elem;
    }
}
// every column but the counter moved by delta bytes (the same table seen through another mapping of its memory)
inline fg_tables shifted(const fg_tables& t, ptrdiff_t delta) {
    fg_tables r = t;
    for (int k = 0; k < FG_TABLE_ARRAYS; ++k)
        if (kTableCols[k].kind != COL_COUNTER) set_col(&r, k, col(t, k) + delta);
    return r;
}
// rows [r0, r0 + rows) of t as a table of their own: the entry columns and the counter stay shared
inline fg_tables rows_of(const fg_tables& t, uint64_t r0, uint64_t rows) {
    fg_tables r = t;
    r.n = rows;
    for (int k = 0; k < FG_TABLE_ARRAYS; ++k)
        if (kTableCols[k].kind == COL_ROW) set_col(&r, k, col(t, k) + r0 * kTableCols[k].elem);
    return r;
}
inline bool has_cols(const fg_tables& t, ColKind kind) {
    for (int k = 0; k < FG_TABLE_ARRAYS; ++k)
        if (kTableCols[k].kind == kind && !col(t, k)) return false;
    return true;
}
inline bool has_rows(const fg_tables& t) { return has_cols(t, COL_ROW); }
inline bool has_entries(const fg_tables& t) { return has_cols(t, COL_ENT); }

}  // namespace fg
