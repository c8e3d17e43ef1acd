// fg_ctx.hpp -- private to the host side of the C ABI (fg_capi.cpp: contexts + the device entry points; fg_host_pipeline.cpp: the
// PCIe-inclusive host-buffer entry points): the ctx, the kernel launchers' prototypes and the small helpers both translation units use.
// Not installed, not part of the ABI (include/fg_hip.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "../../include/fg_hip.h"
#include "fg_cus.hpp"
#include "fg_device.hpp"
#include "fg_enc_cfg.hpp"
#include "fg_fused_plan.hpp"
#include "fg_table_cols.hpp"
#include <time.h>

#include "fg_rfc3164_parse.hpp"
#include "fg_tz_index.hpp"

namespace fg {
// device view of input.ltsv_schema / input.ltsv_suffixes (must match fg_ltsv.hip)
struct LtsvDevCfg {
    uint32_t n_schema;
    const uint8_t* blob;
    const uint32_t* name_off;
    const uint8_t* types;
    uint32_t suf_off[4];
    uint32_t suf_len[4];
    uint32_t has_suf[4];
};
}  // namespace fg

extern "C" int fg_launch_rfc5424(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const fg::DevTables* t,
                                 uint64_t avg_len, hipStream_t stream, uint64_t* stash, uint32_t stash_blocks, uint32_t strip,
                                 const uint8_t* line_bad, const fg_launch_opts* lo, fg::TicketSlot* tk);
extern "C" uint64_t fg_stash_bytes(uint32_t blocks);
extern "C" int fg_launch_rfc3164(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const fg::DevTables* t,
                                 const fg::r3164::Cfg* cfg, uint32_t tile_cap, hipStream_t stream, uint32_t strip,
                                 const uint8_t* line_bad, uint8_t* scratch, int regroup);
// (a WEAK reference: the CPU suite links the host side of the C ABI against fake launchers -- tests/native/host_pipeline_fake.cpp --
//  which have none for this format; FG_CAPNP then answers FG_ERR_UNSUPPORTED.  The product library always has the kernel.)
extern "C" int fg_launch_capnp(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const fg::DevTables* t, uint64_t avg_len,
                               hipStream_t stream, const uint8_t* line_bad, const fg_launch_opts* lo, fg::TicketSlot* tk) __attribute__((weak));
extern "C" uint64_t fg_rfc3164_scratch_bytes(uint64_t n);
extern "C" uint64_t fg_rfc3164_regroup_from(void);   // lines from which the library regroups by itself  // the regrouped form's scratch: shape keys, block counts, the line permutation
extern "C" int fg_launch_encode_sizes(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const fg::DevTables* t,
                                      const fg::EncCfg* cfg, uint32_t tile_cap, uint32_t cfg_lds, uint32_t* d_sizes,
                                      uint64_t* d_block_sums, uint8_t* d_status, uint64_t* d_out_offsets, hipStream_t stream);
extern "C" int fg_launch_encode_count(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const fg::DevTables* t,
                                      const fg::EncCfg* cfg, uint32_t tile_cap, uint32_t cfg_lds, uint32_t* d_sizes,
                                      uint64_t* d_block_sums, uint8_t* d_status, hipStream_t stream);
extern "C" int fg_launch_encode_scan(const uint32_t* d_sizes, uint64_t* d_block_sums, uint64_t n, uint64_t* d_out_offsets, uint64_t base,
                                     hipStream_t stream);
extern "C" int fg_launch_encode_write(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const fg::DevTables* t,
                                      const fg::EncCfg* cfg, uint32_t tile_cap, uint32_t cfg_lds, const uint64_t* d_out_offsets,
                                      uint8_t* d_out, const uint32_t* d_sizes, hipStream_t stream);
extern "C" uint64_t fg_frame_scratch_bytes(uint64_t nbytes);
extern "C" int fg_launch_frame(const uint8_t* d_bytes, uint64_t nbytes, uint32_t delim, uint8_t* scratch, uint64_t* d_offsets,
                               uint8_t* d_bad, uint64_t cap, uint64_t** d_total_out, hipStream_t stream, int classic);
constexpr uint64_t FG_FRAME_ABORTED = ~0ull;  // *d_total_out after a one-pass launch whose look-back gave up: launch again, classic
// the octet-counted framer (fg_syslen.hip): *d_hdr_out = its result words in device memory (fg::syslen H_*).  (WEAK references, as
// fg_launch_capnp above: the fake launchers of the CPU suite have none, fg_frame_syslen_device then answers FG_ERR_UNSUPPORTED and the
// host-buffer entry points take their host hop.  The product library always has the kernels: build.py checks the link.)
extern "C" uint64_t fg_syslen_scratch_bytes(uint64_t nbytes) __attribute__((weak));
extern "C" uint64_t fg_syslen_max_bytes(void) __attribute__((weak));
extern "C" int fg_launch_syslen(const uint8_t* d_bytes, uint64_t nbytes, uint8_t* scratch, uint8_t* d_packed, uint64_t* d_offsets,
                                uint64_t* d_starts, uint8_t* d_bad, uint64_t cap, uint32_t** d_hdr_out, hipStream_t stream) __attribute__((weak));
// the Cap'n Proto stream framer (fg_capnp_frame.hip): *d_hdr_out = its result words in device memory (fg::capnpf H_*).  (WEAK references,
// as fg_launch_syslen above: without the kernels fg_frame_capnp_device answers FG_ERR_UNSUPPORTED and the host-buffer entry points walk
// the segment tables on the host.  The product library always has them: build.py checks the link.)
extern "C" uint64_t fg_capnp_frame_scratch_bytes(uint64_t nbytes) __attribute__((weak));
extern "C" uint64_t fg_capnp_frame_max_bytes(void) __attribute__((weak));
extern "C" int fg_launch_capnp_frame(const uint8_t* d_bytes, uint64_t nbytes, uint8_t* scratch, uint64_t* d_offsets, uint64_t cap,
                                     uint32_t** d_hdr_out, hipStream_t stream) __attribute__((weak));
// the UDP input's unpacker (fg_udp.hip): count (sizes + per-64 sums; the scan between the two is fg_launch_encode_scan), then write and
// finish into the slots.  (WEAK references, as fg_launch_syslen above: without the kernels fg_udp_unpack_device answers
// FG_ERR_UNSUPPORTED.  The product library always has them: build.py checks the link.)
extern "C" int fg_launch_udp_count(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint32_t max_inflated, uint32_t* d_sizes,
                                   uint64_t* d_block_sums, uint8_t* d_status, uint8_t* d_drop, hipStream_t stream) __attribute__((weak));
extern "C" int fg_launch_udp_write(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out,
                                   uint64_t out_cap, uint8_t* d_status, uint8_t* d_drop, hipStream_t stream) __attribute__((weak));
extern "C" int fg_launch_udp_finish(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out,
                                    uint64_t out_cap, uint8_t* d_status, uint8_t* d_drop, hipStream_t stream) __attribute__((weak));
// ... and its one-walk form: stage (capacities, their scan, the walk, the scan of the sizes), the write walk for the spilled rows, pack.
// (WEAK references as above: without them fg_udp_unpack_once_device and fg_udp_transcode_batch answer FG_ERR_UNSUPPORTED.)
extern "C" uint64_t fg_udp_stage_bytes(uint64_t nbytes, uint64_t n) __attribute__((weak));
extern "C" int fg_launch_udp_stage(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint32_t max_inflated, uint32_t* d_stage_sizes,
                                   uint64_t* d_stage_sums, uint64_t* d_stage_off, uint8_t* d_stage, uint64_t stage_cap, uint32_t* d_sizes,
                                   uint64_t* d_block_sums, uint64_t* d_out_offsets, uint8_t* d_status, uint8_t* d_drop, uint8_t* d_spilled,
                                   uint32_t* d_n_spilled, hipStream_t stream) __attribute__((weak));
extern "C" int fg_launch_udp_write_spilled(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out,
                                           uint64_t out_cap, uint8_t* d_status, uint8_t* d_drop, const uint8_t* d_spilled, hipStream_t stream) __attribute__((weak));
extern "C" int fg_launch_udp_pack(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out,
                                  uint64_t out_cap, uint8_t* d_status, uint8_t* d_drop, const uint8_t* d_stage, const uint64_t* d_stage_off,
                                  uint64_t stage_cap, const uint8_t* d_spilled, hipStream_t stream) __attribute__((weak));
// the segmented framer (fg_frame_multi.hip): *d_result = two device words, the delimiter count (FG_FRAME_ABORTED: launch again, classic)
// and the slot count.  (WEAK references, as fg_launch_syslen above: without the kernels fg_frame_multi_device answers
// FG_ERR_UNSUPPORTED.  The product library always has them: build.py checks the link.)
extern "C" uint64_t fg_frame_multi_scratch_bytes(uint64_t nbytes, uint64_t n_segs) __attribute__((weak));
extern "C" int fg_launch_frame_multi(const uint8_t* d_bytes, uint64_t nbytes, uint32_t delim, const uint64_t* d_seg_starts, const uint8_t* d_seg_final,
                                     uint64_t n_segs, uint8_t* scratch, uint64_t* d_offsets, uint8_t* d_kind, uint64_t cap, uint64_t* d_seg_first,
                                     uint64_t* d_seg_consumed, uint64_t** d_result, hipStream_t stream, int classic) __attribute__((weak));
// the segmented octet-counted framer (fg_syslen_multi.hip): *d_hdr_out = its result words in device memory (fg::syslen H_DECLINE,
// H_NFRAMES, H_TOTAL, H_DONE).  (WEAK references, as fg_launch_syslen above: without the kernels fg_frame_syslen_multi_device answers
// FG_ERR_UNSUPPORTED and fg_frame_decode_syslen_multi_batch takes its host hop.  The product library always has them: build.py checks
// the link.)
extern "C" uint64_t fg_syslen_multi_scratch_bytes(uint64_t nbytes, uint64_t n_segs) __attribute__((weak));
extern "C" int fg_launch_syslen_multi(const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_seg_starts, uint64_t n_segs, uint8_t* scratch,
                                      uint8_t* d_packed, uint64_t* d_offsets, uint64_t* d_starts, uint8_t* d_bad, uint64_t cap,
                                      uint64_t* d_seg_first, uint64_t* d_seg_consumed, uint8_t* d_seg_stop, uint32_t** d_hdr_out,
                                      hipStream_t stream) __attribute__((weak));
// ... and the per-segment cut behind the first payload that is not UTF-8 (fg_syslen_multi.hip: d_bad 0 / 1 -> FG_SLOT_UNREACHED behind
// each segment's first 1; d_cut = fg_syslen_cut_scratch_bytes(n_segs) bytes).  (WEAK references: without the kernels
// fg_transcode_multi_batch computes the cut on the host from the mirrored verdicts.  The product library always has them.)
extern "C" uint64_t fg_syslen_cut_scratch_bytes(uint64_t n_segs) __attribute__((weak));
extern "C" int fg_launch_syslen_cut(uint8_t* d_bad, uint64_t n, const uint64_t* d_seg_first, uint64_t n_segs, uint32_t* d_cut,
                                    hipStream_t stream) __attribute__((weak));
// the segmented Cap'n Proto framer (fg_capnp_frame_multi.hip): *d_hdr_out = its result words in device memory (fg::capnpf H_DECLINE,
// H_NFRAMES = the slots, H_DONE).  (WEAK references, as fg_launch_syslen above: without the kernels fg_frame_capnp_multi_device answers
// FG_ERR_UNSUPPORTED and fg_frame_decode_capnp_multi_batch walks the segments on the host.  The product library always has them:
// build.py checks the link.)
extern "C" uint64_t fg_capnp_frame_multi_scratch_bytes(uint64_t nbytes, uint64_t n_segs) __attribute__((weak));
extern "C" int fg_launch_capnp_frame_multi(const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_seg_starts, uint64_t n_segs, uint8_t* scratch,
                                           uint64_t* d_offsets, uint8_t* d_kind, uint64_t cap, uint64_t* d_seg_first, uint64_t* d_seg_consumed,
                                           uint8_t* d_seg_stop, uint32_t** d_hdr_out, hipStream_t stream) __attribute__((weak));
// the output compressor (fg_deflate.hip): count (the members' blocks, their scan), blocks (every block into its slot), sizes (the
// members' sizes, their scan), pack; and the member cuts over an encoder's offsets.  (WEAK references, as fg_launch_syslen above: without
// the kernels fg_deflate_device answers FG_ERR_UNSUPPORTED, and so do the transcode entry points of a ctx with compression set.  The
// product library always has them: build.py checks the link.)
extern "C" uint64_t fg_deflate_slot_bytes(uint64_t nbytes, uint64_t n_blocks) __attribute__((weak));
extern "C" int fg_launch_deflate_count(const uint64_t* d_cuts, uint64_t n_members, uint64_t nbytes, uint32_t* d_nblk, uint64_t* d_sums,
                                       uint64_t* d_blk_first, uint32_t* d_err, hipStream_t stream) __attribute__((weak));
extern "C" int fg_launch_deflate_blocks(const uint8_t* d_bytes, const uint64_t* d_cuts, const uint64_t* d_blk_first, uint64_t n_members,
                                        uint64_t n_blocks, uint8_t* d_slots, uint64_t slots_cap, uint32_t* d_blk_size, uint32_t* d_blk_crc,
                                        uint32_t* d_ticket, int cus, hipStream_t stream) __attribute__((weak));
extern "C" int fg_launch_deflate_blocks_dyn(const uint8_t* d_bytes, const uint64_t* d_cuts, const uint64_t* d_blk_first, uint64_t n_members,
                                            uint64_t n_blocks, uint8_t* d_slots, uint64_t slots_cap, uint32_t* d_blk_size, uint32_t* d_blk_crc,
                                            uint32_t* d_ticket, int cus, hipStream_t stream) __attribute__((weak));  // FG_DEFLATE_DYNAMIC
extern "C" int fg_launch_deflate_sizes(const uint64_t* d_cuts, const uint64_t* d_blk_first, uint64_t n_members, const uint32_t* d_blk_size,
                                       const uint32_t* d_blk_crc, uint32_t* d_blk_rel, uint32_t* d_member_crc, uint32_t* d_msize, uint64_t* d_sums,
                                       uint64_t* d_z_offsets, hipStream_t stream) __attribute__((weak));
extern "C" int fg_launch_deflate_pack(const uint8_t* d_bytes, const uint64_t* d_cuts, const uint64_t* d_blk_first, uint64_t n_members, uint64_t n_blocks,
                                      const uint8_t* d_slots, const uint32_t* d_blk_size, const uint32_t* d_blk_rel, const uint32_t* d_member_crc,
                                      const uint64_t* d_z_offsets, uint8_t* d_z, uint64_t z_cap, hipStream_t stream) __attribute__((weak));
extern "C" int fg_launch_deflate_cuts(const uint64_t* d_off, uint64_t n, uint64_t coalesce, uint64_t member_bytes, uint32_t* d_flags, uint64_t* d_sums,
                                      uint64_t* d_idx, uint64_t* d_member_first, uint64_t* d_cuts, uint64_t* d_n_members, hipStream_t stream)
    __attribute__((weak));
// Kafka v0 message sets (fg_kafka.hip): sizes (the messages' wire sizes, their scan), write (header, CRC-32 and value per message), cuts
// (the members' bounds in the set); wrap_sizes (the wrappers' sizes and pieces, their scans), wrap (the members into their wrapper
// messages).  (WEAK references, as the compressor's above: without the kernels fg_kafka_messageset_device and fg_kafka_wrap_device answer
// FG_ERR_UNSUPPORTED, and so do the transcode entry points of a ctx with FG_WIRE_KAFKA_V0 set.  build.py checks the link.)
extern "C" int fg_launch_kafka_sizes(const uint64_t* d_off, const uint8_t* d_skip, uint64_t n, uint64_t nbytes, uint32_t* d_sizes, uint64_t* d_sums,
                                     uint64_t* d_set_offsets, uint32_t* d_err, hipStream_t stream) __attribute__((weak));
extern "C" int fg_launch_kafka_write(const uint8_t* d_bytes, const uint64_t* d_off, const uint8_t* d_skip, uint64_t n, const uint64_t* d_set_offsets,
                                     uint8_t* d_set, uint64_t set_cap, int cus, hipStream_t stream) __attribute__((weak));
extern "C" int fg_launch_kafka_cuts(const uint64_t* d_set_offsets, const uint64_t* d_member_first, uint64_t n, uint64_t n_members, uint64_t* d_set_cuts,
                                    hipStream_t stream) __attribute__((weak));
extern "C" int fg_launch_kafka_wrap_sizes(const uint64_t* d_z_offsets, uint64_t n_members, uint32_t* d_wsize, uint32_t* d_npiece, uint64_t* d_sums,
                                          uint64_t* d_w_offsets, uint64_t* d_piece_first, uint32_t* d_err, hipStream_t stream) __attribute__((weak));
extern "C" int fg_launch_kafka_wrap(const uint8_t* d_z, const uint64_t* d_z_offsets, const uint64_t* d_piece_first, uint64_t n_members, uint64_t n_pieces,
                                    const uint64_t* d_w_offsets, uint8_t* d_w, uint64_t w_cap, uint32_t* d_piece_crc, int cus, hipStream_t stream)
    __attribute__((weak));
extern "C" uint64_t fg_frame_block_bytes(void);
extern "C" uint64_t fg_frame_slice_align(void);
extern "C" int fg_launch_frame_slice(const uint8_t* d_bytes, uint64_t nbytes, uint32_t delim, uint8_t* scratch, uint64_t* d_offsets,
                                     uint8_t* d_bad, uint64_t cap, uint64_t blk0, uint64_t blk1, uint64_t** d_total_out,
                                     hipStream_t stream, const uint8_t* src, int classic);
extern "C" int fg_launch_ltsv(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const fg::DevTables* t,
                              const fg::LtsvDevCfg* cfg, uint64_t avg_len, hipStream_t stream, uint64_t* stash,
                              uint32_t stash_blocks, uint32_t strip, const uint8_t* line_bad, const fg_launch_opts* lo, fg::TicketSlot* tk);
extern "C" int fg_launch_gelf_general(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const fg::DevTables* t, hipStream_t stream,
                                      uint32_t strip, const uint8_t* line_bad);
extern "C" int fg_launch_gelf(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const fg::DevTables* t,
                              uint64_t avg_len, hipStream_t stream, uint64_t* stash, uint32_t stash_blocks, uint32_t strip,
                              const uint8_t* line_bad, const fg_launch_opts* lo, fg::TicketSlot* tk);

extern "C" int fg_launch_gelf_general_dev(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const fg::DevTables* t, hipStream_t stream,
                                          uint32_t strip, const uint8_t* line_bad, const unsigned long long* n_dev);
// the fused launches (fg_fused.hpp): frame + decode of a raw stream chunk in ONE kernel; g from fg::fused_geometry, scratch of
// fg::fused_scratch_bytes(nbytes, g->S) bytes; *d_total = the launch's two result words (lines, abort flag), device memory
extern "C" int fg_launch_rfc5424_fused(const uint8_t* d_bytes, uint64_t nbytes, const fg::DevTables* t, const fg::FusedGeom* g, hipStream_t stream,
                                       uint64_t* stash, uint32_t stash_blocks, uint32_t strip, int final_, uint64_t* d_offsets, uint64_t cap,
                                       uint8_t* scratch, const fg_launch_opts* lo, unsigned long long** d_total);
extern "C" int fg_launch_ltsv_fused(const uint8_t* d_bytes, uint64_t nbytes, const fg::DevTables* t, const fg::LtsvDevCfg* cfg, const fg::FusedGeom* g,
                                    hipStream_t stream, uint64_t* stash, uint32_t stash_blocks, uint32_t strip, int final_, uint64_t* d_offsets,
                                    uint64_t cap, uint8_t* scratch, const fg_launch_opts* lo, unsigned long long** d_total);
extern "C" int fg_launch_gelf_fused(const uint8_t* d_bytes, uint64_t nbytes, const fg::DevTables* t, const fg::FusedGeom* g, hipStream_t stream,
                                    uint32_t strip, int final_, uint64_t* d_offsets, uint64_t cap, uint8_t* scratch, const fg_launch_opts* lo,
                                    unsigned long long** d_total);
extern "C" int fg_launch_poke64(const uint64_t* d_src, uint64_t* dst_devview, hipStream_t stream);
extern "C" uint64_t fg_merge_scratch_bytes(uint64_t rows);
extern "C" int fg_launch_merge_device(const fg_tables* parts, uint32_t g, const uint64_t* const* d_index, const fg_tables* out, uint8_t* d_src_part,
                                      uint64_t max_rows, uint8_t* scratch, hipStream_t stream);
extern "C" int fg_launch_calib(int mode, const uint8_t* d_src, uint8_t* d_dst, uint64_t nbytes, uint32_t* d_sink, hipStream_t stream);

struct fg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // the pipelined host paths (created on first use): uploads
    hipStream_t stream3 = nullptr;  // ... downloads
    std::vector<hipEvent_t> ev_slice;  // ... two events per slice: uploaded, decoded
    hipStream_t s_up = nullptr, s_down = nullptr, s_run = nullptr;  // ... which of the three does what
    hipEvent_t ev_ready = nullptr;
    int last_hip = 0;
    fg_launch_opts lo{};  // launch-geometry overrides (fg_set_launch_opts); all zero = the library's own choices
    uint32_t link_bound_waves = 0;  // host pipelines whose tables lie across the link: waves per CU of the decode grid for the duration of
                                    // a call, where the caller's options leave the choice to the library (fg_host_pipeline.cpp LinkBoundGrid)
    uint32_t table_shares = 0;  // a sliced host path: the launches of the batch that share one entry table (fg::entry_chunk), else 0
    int last_host_path = 0;  // fg_last_host_path: which form the last host-buffer decode call took (FG_PATH_*)
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool ev_valid = false;
    // LTSV configuration (owned copies)
    std::vector<std::string> schema_names;
    std::vector<uint8_t> schema_types;
    std::string suffix[4];
    bool has_suffix[4] = {false, false, false, false};
    uint8_t* d_cfg = nullptr;  // device copy of the LTSV configuration (blob | name_off | types)
    // per-wave scratch where entries (SD pairs / LTSV pairs / GELF extras) are parked between the
    // parse and the copy into the entry table (allocated on the first decode; 8 waves on every CU)
    uint64_t* d_stash = nullptr;
    uint64_t* d_stash2 = nullptr;  // ... of the launches with lane = 1 (fg_decode_frames_impl)
    uint32_t stash_blocks = 0;
    static constexpr uint32_t kPendingRing = 1024;
    uint32_t* d_pending = nullptr;  // ring of kPendingRing hand-over words (DevTables::pending), zeroed once
    uint32_t* d_ticket = nullptr;   // ring of ticket counters, one per decode launch (fg::TicketSlot); zeroed once
    std::vector<uint32_t> h_ticket; // ... what each word holds once the launches issued so far have run
    uint32_t ticket_seq = 0;        // ... the next launch's slot
    uint32_t epoch = 0;             // launch counter of this ctx
    bool defer_general = false;     // a sliced host path: GELF's exact form runs once, behind the last slice (fg_finish_deferred_general)
    uint32_t batch_epoch = 0;       // ... and the slices share one hand-over word: the epoch of the batch's first GELF launch
    uint8_t* d_merge = nullptr;     // fg_merge_tables_device: the scan's scratch (dense offsets, block sums, part tags)
    uint64_t d_merge_cap = 0;
    uint32_t* d_sink = nullptr;     // fg_calibrate_device: the word the read-only sweep may write
    uint64_t* d_used = nullptr;     // fg_decode_batch, zero-copy form: the entry counter (the tables themselves are pinned host memory)
    uint8_t* d_frame = nullptr;  // fg_frame_device scratch (delimiter / UTF-8 masks, block counts)
    uint64_t d_frame_cap = 0;
    uint8_t* d_r3164 = nullptr;  // FG_RFC3164, lines regrouped by shape: keys, block counts, permutation (fg_rfc3164.hip)
    uint64_t d_r3164_cap = 0;
    uint8_t* d_fused = nullptr;  // fg_frame_decode_device: the fused launch's scratch (ticket counters, tile counts, block prefixes)
    uint64_t d_fused_cap = 0;
    uint8_t* d_sl_packed = nullptr;  // FG_FRAME_SYSLEN host-buffer calls: the payloads packed back to back
    uint64_t d_sl_packed_cap = 0;
    uint64_t* d_sl_starts = nullptr; // ... the frame starts in the caller's chunk
    uint64_t d_sl_starts_cap = 0;
    int last_syslen_stop = 0;        // fg_last_syslen_stop
    int last_capnp_stop = 0;         // fg_last_capnp_stop
    uint64_t last_syslen_payload = 0; // fg_frame_syslen_device: the payload bytes its last call packed (the host-buffer calls size the decode with it)
    // fg_udp_decode_batch also BORROWS d_bytes (the datagrams), d_sl_packed (the payloads), d_offsets (their offsets), d_bad (the drop
    // flags) and d_tab / h_tab from the frame / syslen / decode paths: every host-buffer call on a ctx synchronises before it returns,
    // so no two of them have these buffers in use at once.
    uint8_t* d_udp = nullptr;        // the unpackers' per-datagram scratch: UdpSizes (fg_udp_unpack_device) or UdpOnce (the one-walk form), fg_capi.cpp
    uint64_t d_udp_cap = 0;
    uint8_t* d_udp_stage = nullptr;  // fg_udp_unpack_once_device: the stages the one walk inflates into
    uint64_t d_udp_stage_cap = 0;
    uint32_t udp_last_spilled = 0;   // fg_udp_last_spilled (a word the front half downloads into)
    uint64_t* d_udp_off = nullptr;   // fg_udp_decode_batch: the datagrams' offsets
    uint64_t d_udp_off_cap = 0;
    uint8_t* d_udp_st = nullptr;     // ... their fg_udp_status
    uint64_t d_udp_st_cap = 0;
    uint8_t* h_udp = nullptr;        // ... pinned: inflated lines | their offsets | fg_udp_status
    uint64_t h_udp_cap = 0;
    uint8_t* d_ms = nullptr;         // the multi-connection host entries: the per-segment device columns (SegBatch, fg_host_pipeline.cpp)
    uint64_t d_ms_cap = 0;
    uint8_t* h_ms = nullptr;         // ... pinned: the mirror their out_* pointers name
    uint64_t h_ms_cap = 0;
    uint8_t* d_bad = nullptr;    // fg_frame_decode_batch: per-frame UTF-8 verdicts
    uint64_t d_bad_cap = 0;
    uint64_t* h_off = nullptr;   // fg_frame_decode_batch: pinned host copy of the frame offsets
    uint64_t h_off_cap = 0;
    uint64_t* h_cnt = nullptr;   // ... pinned words the pipelined form reads the slices' frame counts through
    double frames_per_byte = 1.0 / 200.0;  // ... what the last raw chunk held (sizes the next one's tables before its frames are counted)
    // RFC3164 configuration: host copies (for fg_clone) + one device block [names | name_off | zone_first | utc_start | utc_off]
    bool r3164_set = false;
    bool r3164_auto_year = false;  // current_year == FG_YEAR_NOW: follow the wall clock like the reference (:179)
    int32_t r3164_year = 1970;
    std::vector<uint8_t*> retired_tz;  // zone blocks replaced at a year change (kernels may still read them; freed at destroy)
    std::vector<std::string> tz_names;
    std::vector<uint32_t> tz_first;
    std::vector<int64_t> tz_start;
    std::vector<int32_t> tz_off;
    uint8_t* d_tz = nullptr;
    fg::r3164::Cfg r3164{};
    uint8_t* d_enc = nullptr;    // fg_encode_gelf_device: static key list + blob, then the per-line sizes
    uint64_t d_enc_cap = 0;
    // fg_encode_device_async: pinned ring the encoder configuration is uploaded from without a host sync
    static constexpr uint32_t kEncRing = 4, kEncSlot = 16 * 1024;
    uint8_t* h_enc_ring = nullptr;
    hipEvent_t ev_enc[kEncRing] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t enc_ring_next = 0;
    fg::LtsvDevCfg ltsv{};
    // staging for fg_decode_batch
    uint8_t* d_bytes = nullptr;
    uint64_t d_bytes_cap = 0;
    uint64_t* d_offsets = nullptr;
    uint64_t d_offsets_cap = 0;
    uint8_t* d_tab = nullptr;  // one device allocation carved into the table arrays
    uint64_t d_tab_cap = 0;
    uint8_t* h_tab = nullptr;  // pinned host mirror
    uint64_t h_tab_cap = 0;
    // fg_transcode_batch: device output (messages | out_offsets | enc_status) and its pinned host mirror
    uint8_t* d_tout = nullptr;
    uint64_t d_tout_cap = 0;
    uint8_t* d_tmeta = nullptr;  // out_offsets[n + 1] then enc_status[n]
    uint64_t d_tmeta_cap = 0;
    uint8_t* h_tout = nullptr;   // pinned: messages | out_offsets | meta | enc_status
    uint64_t h_tout_cap = 0;
    // the output compressor (fg_deflate_device, and behind the encoder of the transcode entry points: fg_set_output_compression)
    fg_compress_cfg compress{FG_COMP_NONE, 1u, 0u};
    int deflate_mode = FG_DEFLATE_FIXED;  // fg_set_deflate_mode
    fg_compressed last_comp{};       // fg_last_compressed
    uint8_t* d_df = nullptr;         // per member: DfMembers (fg_capi.cpp)
    uint64_t d_df_cap = 0;
    uint8_t* d_df_blk = nullptr;     // per block: DfBlocks (fg_capi.cpp)
    uint64_t d_df_blk_cap = 0;
    uint8_t* d_df_slots = nullptr;   // the slots the blocks are compressed into
    uint64_t d_df_slots_cap = 0;
    uint64_t df_blocks = 0;          // ... how many of them the last front half found (a word it downloads into)
    uint32_t df_err = 0;             // ... and whether it refused the cuts
    uint8_t* d_df_cut = nullptr;     // the transcode entry points' member stage: MemberCuts (fg_host_pipeline.cpp)
    uint64_t d_df_cut_cap = 0;
    uint64_t df_members = 0;         // ... the members of the last cut (a word it is downloaded into)
    uint8_t* d_zout = nullptr;       // ... the compressed stream
    uint64_t d_zout_cap = 0;
    uint8_t* h_zout = nullptr;       // ... pinned: the members | z_offsets | member_first
    uint64_t h_zout_cap = 0;
    // Kafka v0 message sets (fg_kafka_messageset_device, fg_kafka_wrap_device, and behind the encoder of the transcode entry points:
    // fg_set_output_wire)
    int wire = FG_WIRE_RAW;
    uint8_t* d_kf = nullptr;         // per message: KfSet (fg_capi.cpp)
    uint64_t d_kf_cap = 0;
    uint8_t* d_kf_wrap = nullptr;    // per member: KfWrap (fg_capi.cpp)
    uint64_t d_kf_wrap_cap = 0;
    uint8_t* d_kf_crc = nullptr;     // per piece: its CRC register
    uint64_t d_kf_crc_cap = 0;
    uint32_t kf_err = 0;             // whether the last front half refused its offsets (a word it downloads into)
    uint64_t kf_pieces = 0;          // ... and the pieces the last wrap front found
    uint8_t* d_kf_set = nullptr;     // the transcode entry points: the message set
    uint64_t d_kf_set_cap = 0;
    uint8_t* d_kf_off = nullptr;     // ... the offset lists of the member stage: KfOffsets (fg_host_pipeline.cpp)
    uint64_t d_kf_off_cap = 0;
    uint8_t* d_kf_w = nullptr;       // ... the wrapper messages
    uint64_t d_kf_w_cap = 0;
};

namespace {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

#define FG_HIP(ctx, call)                         \
    do {                                          \
        hipError_t e_ = (call);                   \
        if (e_ != hipSuccess) {                   \
            (ctx)->last_hip = (int)e_;            \
            return FG_ERR_HIP;                    \
        }                                         \
    } while (0)
// ... and for the kernel launchers (fg_launch_*: 0, or what went wrong as an int)
#define FG_LAUNCH(ctx, call)                      \
    do {                                          \
        const int l_ = (call);                    \
        if (l_ != 0) {                            \
            (ctx)->last_hip = l_;                 \
            return FG_ERR_HIP;                    \
        }                                         \
    } while (0)

// the stream a call runs on: the caller's, or the ctx's own
inline hipStream_t stream_of(const fg_ctx* ctx, void* stream) { return stream == FG_STREAM_OWN ? ctx->stream : (hipStream_t)stream; }

inline uint64_t up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// carve `base` into the arrays of an fg_tables (256-byte aligned pieces)
void carve(uint8_t* base, uint64_t n, uint64_t ent_cap, fg_tables* t, uint64_t* total) {
    uint64_t sizes[FG_TABLE_ARRAYS];
    fg::layout(n, ent_cap, sizes);
    if (t) {
        t->n = n;
        t->ent_cap = ent_cap;
    }
    uint64_t off = 0;
    for (int k = 0; k < FG_TABLE_ARRAYS; ++k) {
        if (t) fg::set_col(t, k, base ? base + off : nullptr);
        off += up(sizes[k], 256);
    }
    if (total) *total = off;
}
inline uint64_t carved_bytes(uint64_t n, uint64_t ent_cap) {
    uint64_t total = 0;
    carve(nullptr, n, ent_cap, nullptr, &total);
    return total;
}

// The entry table of a host-buffer call is sized from the input bytes and grown from what the counter reports (include/fg_hip.h,
// fg_tables::ent_used): one entry per 16 (RFC5424) / 8 input bytes to start with; RFC3164 produces no entries.
constexpr uint64_t kEntCapMax = 0xFFFFFFF0ull;  // (ent_first is 32 bits wide)
inline uint64_t first_ent_cap(fg_format fmt, uint64_t nbytes) {
    if (fmt == FG_RFC3164) return 16;
    return std::min(fmt == FG_RFC5424 ? nbytes / 16 + 1024 : nbytes / 8 + 1024, kEntCapMax);
}
inline uint64_t next_ent_cap(uint64_t used) { return std::min(used + used / 8 + 1024, kEntCapMax); }

fg::DevTables to_dev(const fg_tables& t) {
    fg::DevTables d;
    d.n = t.n;
    d.ent_cap = t.ent_cap;
    d.meta = t.meta;
    d.ts = t.ts;
    d.span[0] = t.hostname;
    d.span[1] = t.appname;
    d.span[2] = t.procid;
    d.span[3] = t.msgid;
    d.span[4] = t.msg;
    d.span[5] = t.full_msg;
    d.ent_first = t.ent_first;
    d.ent_count = t.ent_count;
    d.ent_name = t.ent_name;
    d.ent_val = t.ent_val;
    d.ent_type = t.ent_type;
    d.ent_flags = t.ent_flags;
    d.ent_used = (unsigned long long*)t.ent_used;
    d.pending = nullptr;
    d.epoch = 0;
    d.alloc_chunk = 0;
    d.shares = 1;
    return d;
}

}  // namespace
#include "fg_tile_cap.hpp"
namespace {

int grow_dev(fg_ctx* ctx, void** p, uint64_t* cap, uint64_t need) {
    if (need <= *cap) return FG_OK;
    if (*p) FG_HIP(ctx, hipFree(*p));
    *p = nullptr;
    *cap = 0;
    uint64_t want = up(need + need / 4, 1 << 20);
    FG_HIP(ctx, hipMalloc(p, want));
    *cap = want;
    return FG_OK;
}

int grow_pinned(fg_ctx* ctx, void** p, uint64_t* cap, uint64_t need) {
    if (need <= *cap) return FG_OK;
    if (*p) FG_HIP(ctx, hipHostFree(*p));
    *p = nullptr;
    *cap = 0;
    uint64_t want = up(need + need / 4, 1 << 20);
    FG_HIP(ctx, hipHostMalloc(p, want, hipHostMallocDefault));
    *cap = want;
    return FG_OK;
}

// One scratch allocation handed out array by array.  A layout struct (UdpOnce, DfMembers, MemberCuts, ...) walks its arrays through one
// of these in its constructor and nowhere else: over the buffer for the launchers' pointers, over a null base for the size to ask of
// grow_dev (`Layout(nullptr, n).bytes`), so the two cannot disagree.  take: `count` elements of T, the next array `pad`-aligned behind them.
struct Carver {
    uint8_t* base;
    uint64_t off = 0;
    template <class T>
    T* take(uint64_t count, uint64_t pad = 16) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += up(count * sizeof(T), pad);
        return p;
    }
};

// One framing scan of d_bytes[0 .. nbytes) on s, shared by fg_frame_device and the host paths' frame_stage: the one-pass scan, launched
// again in its classic three-kernel form when its look-back gave up (FG_FRAME_ABORTED).  *total = the delimiters = the terminated
// frames; more of them (and a possible tail) than `cap` holds -> FG_ERR_ENT_OVERFLOW, nothing else is read; else *last_end = where the
// last terminated frame ends (short of nbytes: an unterminated tail follows, whose end the scan has written behind it).
int frame_scan(fg_ctx* ctx, fg_framing framing, const uint8_t* d_bytes, uint64_t nbytes, uint64_t* d_offsets, uint8_t* d_bad, uint64_t cap,
               hipStream_t s, uint64_t* total, uint64_t* last_end) {
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_frame, &ctx->d_frame_cap, fg_frame_scratch_bytes(nbytes))) != FG_OK) return rc;
    for (int classic = (ctx->lo.flags & FG_LO_FRAME_CLASSIC) ? 1 : (ctx->lo.flags & FG_LO_FRAME_SELFTEST_STALL) ? 2 : 0;; classic = 1) {
        uint64_t* d_total = nullptr;
        FG_LAUNCH(ctx, fg_launch_frame(d_bytes, nbytes, framing == FG_FRAME_LINE ? 0x0Au : 0x00u, ctx->d_frame, d_offsets, d_bad, cap, &d_total, s, classic));
        FG_HIP(ctx, hipMemcpyAsync(total, d_total, 8, hipMemcpyDeviceToHost, s));
        FG_HIP(ctx, hipStreamSynchronize(s));
        if (*total != FG_FRAME_ABORTED || classic == 1) break;  // (the one-pass scan gave up waiting on a tile: the three-kernel form)
    }
    if (*total + 1 > cap) return FG_ERR_ENT_OVERFLOW;
    FG_HIP(ctx, hipMemcpyAsync(last_end, d_offsets + *total, 8, hipMemcpyDeviceToHost, s));
    FG_HIP(ctx, hipStreamSynchronize(s));
    return FG_OK;
}

// The encoder kernels' configuration staged for n lines (fg_encode_device, fg_encode_device_async, the sliced fg_transcode_batch).
// ctx->d_enc holds [static keys | blob] -- the IMAGE, image_bytes of it --, then a size per line, then `sum_words` block sums.  The
// image is written to host memory of the caller's (write_image), and the caller copies it to ctx->d_enc: from where, on which stream
// and whether anything waits for it is its business.
struct EncStage {
    fg::EncCfgHost host;
    fg::EncCfg cfg{};              // keys / blob point into ctx->d_enc
    uint32_t cfg_lds = 0;          // the bytes of [static keys | blob] the kernels mirror in LDS when it is small (it nearly always is), else 0
    uint32_t* d_sizes = nullptr;
    uint64_t* d_block_sums = nullptr;
    uint64_t image_bytes = 0, keys_bytes = 0;
    void write_image(uint8_t* dst) const {
        memset(dst, 0, image_bytes);
        if (!host.keys.empty()) memcpy(dst, host.keys.data(), host.keys.size() * sizeof(fg::StaticKey));
        if (!host.blob.empty()) memcpy(dst + keys_bytes, host.blob.data(), host.blob.size());
    }
};
int stage_encoder(fg_ctx* ctx, fg_format src_fmt, const fg_encode_cfg* ecfg, uint64_t n, uint64_t sum_words, EncStage* st) {
    if (!fg::build_enc_cfg(src_fmt, ecfg, ctx->suffix, ctx->has_suffix, &st->host)) return FG_ERR_ARG;
    st->keys_bytes = up(st->host.keys.size() * sizeof(fg::StaticKey), 16);
    st->image_bytes = up(st->keys_bytes + up(st->host.blob.size() + 16, 256), 256);
    const uint64_t sizes_bytes = up(n * 4 + 4, 256);
    const int rc = grow_dev(ctx, (void**)&ctx->d_enc, &ctx->d_enc_cap, st->image_bytes + sizes_bytes + up(sum_words * 8, 256));
    if (rc != FG_OK) return rc;
    st->cfg = st->host.cfg;
    st->cfg.keys = reinterpret_cast<const fg::StaticKey*>(ctx->d_enc);
    st->cfg.blob = ctx->d_enc + st->keys_bytes;
    const uint64_t text = st->keys_bytes + st->host.blob.size();
    st->cfg_lds = text <= 4096 ? (uint32_t)up(text, 16) : 0u;
    st->d_sizes = reinterpret_cast<uint32_t*>(ctx->d_enc + st->image_bytes);
    st->d_block_sums = reinterpret_cast<uint64_t*>(ctx->d_enc + st->image_bytes + sizes_bytes);
    return FG_OK;
}
// the GELF ranking scratch is sized by the pairs per line: `entries` of them in `lines` lines (~0: not known, the largest)
inline void pick_sort_slots(fg::EncCfg* cfg, uint64_t entries, uint64_t lines) {
    if (entries == 0) cfg->sort_slots = 1;                   // no pairs at all (e.g. RFC5424 without structured data)
    else if (entries <= 2 * lines) cfg->sort_slots = 8;      // on average <= 2 pairs per line
}

// ctx->h_cnt: one pinned 64 KiB block of words the pipelined host paths read small results through.  Who owns which words:
constexpr uint32_t kCntWords = 8192;
constexpr uint32_t kCntSlices = 0, kMaxFrameSlices = 4096;  // frame_decode_sliced: the frame count after slice k, one word more for a tail's end
constexpr uint32_t kCntEnts = kCntSlices + kMaxFrameSlices, kMaxDecodeSlices = 256;  // fg_decode_batch: the entry counter after slice k
constexpr uint32_t kCntFused = kCntEnts + kMaxDecodeSlices;  // frame_decode_fused: frames, abort flag, entries
constexpr uint32_t kCntEnd = kCntFused + 256;                // transcode_sliced: where the slice's messages end (a page of its own, as ever)
static_assert(kCntFused + 3 <= kCntEnd && kCntEnd + 1 <= kCntWords && kCntEnd * 8 % 4096 == 0, "the regions of h_cnt overlap or leave the block");
int ensure_h_cnt(fg_ctx* ctx) {
    if (!ctx->h_cnt) FG_HIP(ctx, hipHostMalloc((void**)&ctx->h_cnt, kCntWords * 8, hipHostMallocDefault));
    return FG_OK;
}

// device -> host copies of table columns on `stream`: one hipMemcpyAsync per column, in fg_tables order, nothing for an empty range
int copy_cols(fg_ctx* ctx, const fg_tables& dst, const fg_tables& src, fg::ColKind kind, uint64_t i0, uint64_t cnt, hipStream_t stream) {
    for (int k = 0; k < FG_TABLE_ARRAYS && cnt; ++k) {
        const fg::TableCol& c = fg::kTableCols[k];
        if (c.kind == kind) FG_HIP(ctx, hipMemcpyAsync(fg::col(dst, k) + i0 * c.elem, fg::col(src, k) + i0 * c.elem, cnt * c.elem, hipMemcpyDeviceToHost, stream));
    }
    return FG_OK;
}
int copy_rows(fg_ctx* ctx, const fg_tables& dst, const fg_tables& src, uint64_t r0, uint64_t rows, hipStream_t stream) {
    return copy_cols(ctx, dst, src, fg::COL_ROW, r0, rows, stream);
}
int copy_entries(fg_ctx* ctx, const fg_tables& dst, const fg_tables& src, uint64_t e0, uint64_t e1, hipStream_t stream) {
    return copy_cols(ctx, dst, src, fg::COL_ENT, e0, e1 > e0 ? e1 - e0 : 0, stream);
}
// a whole table: n rows, the first `used` entry slots, the counter
int copy_table(fg_ctx* ctx, const fg_tables& dst, const fg_tables& src, uint64_t n, uint64_t used, hipStream_t stream) {
    int rc;
    if ((rc = copy_rows(ctx, dst, src, 0, n, stream)) != FG_OK || (rc = copy_entries(ctx, dst, src, 0, used, stream)) != FG_OK) return rc;
    return copy_cols(ctx, dst, src, fg::COL_COUNTER, 0, 1, stream);
}

}  // namespace

// one decode launch on `stream` (fg_capi.cpp).  reset_counter = false: a further slice of a batch whose entry counter is already live;
// span_bytes = the bytes the n lines cover (launch geometry is planned from the average line); lane = 1: the launch parks its entries
// in the ctx's second stash and never regroups RFC3164 lines.  (The sliced fg_transcode_batch gives its slices lanes 0 and 1 in turn.
// Its slices once ran on two lanes of streams; they are queued on one stream now, and the argument stays because it also decides
// which RFC3164 kernel runs.)
extern "C" int fg_finish_deferred_general(fg_ctx* ctx, fg_framing framing, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                               const uint8_t* d_bad_utf8, const fg_tables* tables, void* stream);
// the two halves of fg_udp_unpack_once_device (fg_capi.cpp), for fg_udp_transcode_batch, which sizes its buffer between them: the front
// walks every datagram once and synchronises for *total, the pack fills d_out[0 .. out_cap) (out_cap >= *total) and is not waited for
extern "C" int fg_udp_once_front(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_offsets, uint64_t n, uint64_t max_inflated,
                                 uint64_t* d_out_offsets, uint8_t* d_drop, uint8_t* d_udp_status, uint64_t* total, hipStream_t s);
extern "C" int fg_udp_once_pack(fg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out,
                                uint64_t out_cap, uint8_t* d_drop, uint8_t* d_udp_status, hipStream_t s);
// the two halves of fg_deflate_device (fg_capi.cpp), for member_stage (fg_host_pipeline.cpp), which sizes its buffer between them: the front compresses
// every block into ctx-owned slots, leaves d_z_offsets[n_members + 1] and synchronises for *total; the pack fills d_z[0 .. z_cap)
// (z_cap >= *total) and is not waited for.  n_members > 0.
extern "C" int fg_deflate_front(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_cuts, uint64_t n_members, uint64_t* d_z_offsets,
                                uint64_t* total, hipStream_t s);
extern "C" int fg_deflate_pack(fg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_cuts, uint64_t n_members, const uint64_t* d_z_offsets, uint8_t* d_z,
                               uint64_t z_cap, hipStream_t s);
// ... and of fg_kafka_messageset_device / fg_kafka_wrap_device, in the same way: a front leaves the offsets and synchronises for *total,
// the write / wrap fills the buffer (its capacity >= *total) and is not waited for.  n > 0, n_members > 0.
extern "C" int fg_kafka_set_front(fg_ctx* ctx, const uint64_t* d_offsets, const uint8_t* d_skip, uint64_t n, uint64_t nbytes, uint64_t* d_set_offsets,
                                  uint64_t* total, hipStream_t s);
extern "C" int fg_kafka_set_write(fg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, const uint8_t* d_skip, uint64_t n,
                                  const uint64_t* d_set_offsets, uint8_t* d_set, uint64_t set_cap, hipStream_t s);
extern "C" int fg_kafka_wrap_front(fg_ctx* ctx, const uint64_t* d_z_offsets, uint64_t n_members, uint64_t* d_w_offsets, uint64_t* total, hipStream_t s);
extern "C" int fg_kafka_wrap_write(fg_ctx* ctx, const uint8_t* d_z, const uint64_t* d_z_offsets, uint64_t n_members, const uint64_t* d_w_offsets, uint8_t* d_w,
                                   uint64_t w_cap, hipStream_t s);
// one fused launch on `stream` (fg_capi.cpp): *d_total = its result words in ctx scratch.  FG_ERR_UNSUPPORTED: nothing was launched
extern "C" int fg_frame_decode_impl(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* d_bytes, uint64_t nbytes, int final,
                                    uint64_t* d_offsets, uint64_t cap, const fg_tables* tables, uint64_t avg_line, void* stream,
                                    unsigned long long** d_total);
extern "C" int fg_decode_frames_impl(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* d_bytes, uint64_t nbytes,
                          const uint64_t* d_offsets, uint64_t n, const uint8_t* d_bad_utf8, const fg_tables* tables,
                          void* stream, bool reset_counter, uint64_t span_bytes, uint32_t lane = 0);
