"""Decoders -- host-side mirror of flowgger's `Decoder` trait for the GPU bulk-parse stage.

Reference interface (src/flowgger/decoder/mod.rs:23-46):

    pub trait Decoder: CloneBoxedDecoder {
        fn decode(&self, line: &str) -> Result<Record, &'static str>;
    }

Same names, same argument meaning, same error strings: ``decode(line)`` returns a
:class:`~flowgger_amd.record.Record` or raises :class:`~flowgger_amd.record.DecodeError` whose
message is the reference's ``&'static str``.  What is new is ``decode_batch`` / ``decode_packed``:
the batching framer hands over N framed lines at once and ONE call runs the gfx950 kernels
(the per-line loop it replaces: src/flowgger/splitter/line_splitter.rs:17,44-54).

Every call goes through the C ABI of libfg_hip.so; there is no CPU implementation here.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib as L
from .record import DecodeError, Record, parse_canonical
from .tables import DeviceTables, HostTables

_TYPE_IDS = {"string": L.FG_T_STRING, "bool": L.FG_T_BOOL, "f64": L.FG_T_F64, "i64": L.FG_T_I64, "u64": L.FG_T_U64}


def pack_lines(lines: Iterable[Union[str, bytes]]) -> Tuple[np.ndarray, np.ndarray]:
    """The batching framer's container: framed lines -> (packed bytes, offsets[n+1] uint64)."""
    bl = [ln.encode("utf-8", "surrogateescape") if isinstance(ln, str) else bytes(ln) for ln in lines]
    offsets = np.zeros(len(bl) + 1, np.uint64)
    if bl:
        offsets[1:] = np.cumsum([len(b) for b in bl], dtype=np.uint64)
    data = np.frombuffer(b"".join(bl), np.uint8).copy() if bl else np.zeros(0, np.uint8)
    return data, offsets


def _copied(ptr, ctype, count: int) -> np.ndarray:
    """`count` elements of a ctx-owned C array as a numpy array of its own; empty for a zero count (the pointer may be NULL then)"""
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (count,)).copy() if count else np.zeros(0, ctype)


def _framed_within(what: str, cap: int, fixed: bool, slack: int, attempt):
    """The capacity of a multi-connection device framer is an estimate: attempt(cap) allocates the tensors sized by it, calls the
    entry and returns (rc, count, tensors).  FG_ERR_ENT_OVERFLOW comes with the count the buffer needs: unless the caller fixed the
    capacity, once more with count + slack.  -> (count, tensors)"""
    while True:
        rc, n, tensors = attempt(cap)
        if rc == L.FG_ERR_ENT_OVERFLOW and not fixed:
            cap = n + slack
            continue
        L.check(rc, what)
        return n, tensors


class Decoder:
    """Base: owns an fg_ctx (the analogue of Box<dyn Decoder + Send>)."""

    fmt: int = -1

    def __init__(self, config: Optional[dict] = None, device: int = 0):
        self._cfg = self._make_cfg(config)
        self._ctx = C.c_void_p()
        self.device = device
        L.check(L.lib().fg_create(device, C.byref(self._cfg) if self._cfg is not None else None,
                                  C.byref(self._ctx)), "fg_create")

    # -- configuration hook (only LTSV has one) ------------------------------------------
    def _make_cfg(self, config: Optional[dict]):
        return None

    def clone_boxed(self) -> "Decoder":  # decoder/mod.rs:29-36
        other = object.__new__(type(self))
        other._cfg = self._cfg
        other._keep = getattr(self, "_keep", None)
        other.device = self.device
        other._ctx = C.c_void_p()
        L.check(L.lib().fg_clone(self._ctx, C.byref(other._ctx)), "fg_clone")
        return other

    def set_launch_opts(self, lines_per_group: int = 0, tile_cap: int = 0, waves_per_cu: int = 0, gelf_lds_budget: int = 0,
                        gelf_window_kib: int = 0, gelf_generic: bool = False, transcode_one_piece: bool = False, chunk_lines: int = 0,
                        no_head: bool = False, force_head: bool = False, sd_walk: bool = False, sd_pairs: bool = False, no_zero_copy: bool = False, frame_kernel_upload: bool = False, frame_classic: bool = False, static_chunks: bool = False, frame_selftest_stall: bool = False, ent_chunk: int = 0, no_taper: bool = False, taper_levels: int = 0, no_fused_framing: bool = False, fused_look: int = 0, fused_ext: int = 0, rfc3164_regroup: int = 0, no_sparse: bool = False, force_sparse: bool = False) -> None:
        """fg_set_launch_opts: launch-geometry overrides of this ctx (parity sweeps over the kernel variants, tuning); 0 = the
        library's own choice.  Results are identical for every setting.  (The library reads no environment variables.)"""
        lo = L.fg_launch_opts(lines_per_group, tile_cap, waves_per_cu, gelf_lds_budget, gelf_window_kib,
                              (L.FG_LO_GELF_GENERIC if gelf_generic else 0) | (L.FG_LO_TRANSCODE_ONE_PIECE if transcode_one_piece else 0) |
                              (L.FG_LO_NO_HEAD if no_head else 0) | (L.FG_LO_FORCE_HEAD if force_head else 0) |
                              (L.FG_LO_SD_WALK if sd_walk else 0) | (L.FG_LO_SD_PAIRS if sd_pairs else 0) | (L.FG_LO_NO_ZERO_COPY if no_zero_copy else 0) | (L.FG_LO_FRAME_KERNEL_UPLOAD if frame_kernel_upload else 0) | (L.FG_LO_FRAME_CLASSIC if frame_classic else 0) | (L.FG_LO_STATIC_CHUNKS if static_chunks else 0) | (L.FG_LO_FRAME_SELFTEST_STALL if frame_selftest_stall else 0) | (L.FG_LO_NO_TAPER if no_taper else 0) | (L.FG_LO_TAPER_1 if taper_levels & 1 else 0) | (L.FG_LO_TAPER_2 if taper_levels & 2 else 0) | (L.FG_LO_NO_FUSED_FRAMING if no_fused_framing else 0) | (L.FG_LO_RFC3164_REGROUP if rfc3164_regroup == 1 else L.FG_LO_RFC3164_NO_REGROUP if rfc3164_regroup == 2 else 0) | (L.FG_LO_NO_SPARSE if no_sparse else 0) | (L.FG_LO_FORCE_SPARSE if force_sparse else 0),
                              chunk_lines, ent_chunk, fused_look, fused_ext)
        L.check(L.lib().fg_set_launch_opts(self._ctx, C.byref(lo)), "fg_set_launch_opts")

    def close(self) -> None:
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            L.lib().fg_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- the reference interface ------------------------------------------------------------
    def decode(self, line: Union[str, bytes]) -> Record:
        res = self.decode_batch([line])[0]
        if isinstance(res, DecodeError):
            raise res
        return res

    # -- bulk interface -----------------------------------------------------------------------
    def decode_packed(self, data: np.ndarray, offsets: np.ndarray) -> HostTables:
        """Host buffers in, host tables out (H2D + kernels + D2H inside the library)."""
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        st = L.fg_tables()
        L.check(L.lib().fg_decode_batch(self._ctx, self.fmt, data.ctypes.data, data.size,
                                        offsets.ctypes.data, n, C.byref(st)), "fg_decode_batch")
        return HostTables.from_struct(st)

    def decode_batch(self, lines: Sequence[Union[str, bytes]]) -> List[Union[Record, DecodeError]]:
        data, offsets = pack_lines(lines)
        raw, offs = self._canonical(self.decode_packed(data, offsets), data, offsets)
        return [parse_canonical(raw[int(offs[i]):int(offs[i + 1])]) for i in range(len(lines))]

    def _canonical(self, tab: HostTables, data: np.ndarray, offsets: np.ndarray, framing: int = L.FG_FRAME_NONE):
        """the rows of `tab` as canonical Record bytes -> (blob bytes, offsets uint64[n + 1]); before that, the decoder's stdout side
        effect (ltsv_decoder.rs:99), reproduced from the rows' flags"""
        if self.fmt == L.FG_LTSV and tab.n and bool(((tab.a["meta"][:tab.n] >> 24) & L.FG_F_LTSV_NOVALUE).any()):
            import sys

            from .tables import tables_stdout

            # (only when a row carries the flag; fg_tables_stdout reads [offsets[i], offsets[i+1]) only: no copy, no slack -- ADVICE r3)
            text = tables_stdout(tab, self.fmt, data, offsets, framing)
            if text:
                sys.stdout.write(text.decode("utf-8", "replace"))
        blob, offs = tab.serialize(self.fmt, data, offsets, cfg=self._cfg)
        return blob.tobytes(), offs

    def decode_device(self, d_bytes, d_offsets, tables: DeviceTables, stream=None) -> None:
        """Device-resident hot path: torch uint8 / int64|uint64 tensors already in HBM.
        Asynchronous on `stream` (a torch.cuda.Stream; default = torch's current stream)."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        n = d_offsets.numel() - 1
        L.check(L.lib().fg_decode_batch_device(self._ctx, self.fmt, d_bytes.data_ptr(), d_bytes.numel(),
                                               d_offsets.data_ptr(), n, C.byref(tables.struct),
                                               C.c_void_p(stream.cuda_stream)), "fg_decode_batch_device")

    # -- GPU framing (the splitter side) -------------------------------------------
    def frame_device(self, d_bytes, framing: int, cap_frames: Optional[int] = None, stream=None):
        """Frame a raw byte stream resident in HBM: `buf_reader.lines()` (framing = FG_FRAME_LINE) or
        `buf_reader.split(0)` (FG_FRAME_NUL) plus the per-frame `str::from_utf8` check
        (splitter/line_splitter.rs:17-25, nul_splitter.rs:18-40).  Returns (d_offsets, d_bad_utf8, n):
        frame i = d_bytes[offsets[i]:offsets[i+1]] INCLUDING its terminator."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        nbytes = d_bytes.numel()
        cap = cap_frames if cap_frames is not None else nbytes // 16 + 16
        while True:
            d_offsets = torch.empty(cap + 2, dtype=torch.int64, device=d_bytes.device)
            d_bad = torch.empty(cap + 1, dtype=torch.uint8, device=d_bytes.device)
            n = C.c_uint64()
            rc = L.lib().fg_frame_device(self._ctx, framing, d_bytes.data_ptr(), nbytes, d_offsets.data_ptr(),
                                         d_bad.data_ptr(), cap, C.byref(n), C.c_void_p(stream.cuda_stream))
            if rc == L.FG_ERR_ENT_OVERFLOW:
                cap = int(n.value) + 16
                continue
            L.check(rc, "fg_frame_device")
            return d_offsets, d_bad, int(n.value)

    def frame_syslen_device(self, d_bytes, final: bool = True, cap_frames: Optional[int] = None, stream=None):
        """Frame an octet-counted stream ("<len> " + len bytes, input.framing = "syslen") resident in HBM: read_msglen + read_exact +
        the per-message String::from_utf8 of SyslenSplitter::run (splitter/syslen_splitter.rs:17-57), FRAMED AND PACKED.  Returns
        (d_packed uint8, d_offsets int64[n + 1] into d_packed -- the FG_FRAME_NONE convention: decode_frames_device / the encoders take
        the two as they are --, d_frame_starts int64[n + 1] into d_bytes with the prefixes, d_bad uint8[n], n, consumed, stop_reason
        (an FG_SYSLEN_*)).  Every payload that is not valid UTF-8 is flagged; the reference panics at the first one, and stopping
        there is the caller's job.  FgError(FG_ERR_UNSUPPORTED) when the device path declines the chunk: frame it on the host.
        d_bytes must start at a 16-byte aligned address (FG_ERR_ARG otherwise: a slice of a tensor from an odd offset does not) and
        its memory must be readable up to numel() rounded up to 16 -- view it into an allocation with that pad."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        nbytes = d_bytes.numel()
        cap = cap_frames if cap_frames is not None else nbytes // 32 + 16
        d_packed = torch.empty((nbytes + 15) // 16 * 16 + 16, dtype=torch.uint8, device=d_bytes.device)
        while True:
            d_offsets = torch.empty(cap + 1, dtype=torch.int64, device=d_bytes.device)
            d_starts = torch.empty(cap + 1, dtype=torch.int64, device=d_bytes.device)
            d_bad = torch.empty(max(cap, 1), dtype=torch.uint8, device=d_bytes.device)
            n, consumed, stop = C.c_uint64(), C.c_uint64(), C.c_int()
            rc = L.lib().fg_frame_syslen_device(self._ctx, d_bytes.data_ptr(), nbytes, int(final), d_packed.data_ptr(), d_offsets.data_ptr(),
                                                d_starts.data_ptr(), d_bad.data_ptr(), cap, C.byref(n), C.byref(consumed), C.byref(stop),
                                                C.c_void_p(stream.cuda_stream))
            if rc == L.FG_ERR_ENT_OVERFLOW:
                cap = int(n.value) + 16
                continue
            L.check(rc, "fg_frame_syslen_device")
            k = int(n.value)
            return d_packed, d_offsets[:k + 1], d_starts[:k + 1], d_bad[:k], k, int(consumed.value), int(stop.value)

    def frame_capnp_device(self, d_bytes, final: bool = True, cap_frames: Optional[int] = None, stream=None):
        """Frame a Cap'n Proto stream resident in HBM (fg_frame_capnp_device): the walk of capnp::serialize::read_message over the
        segment tables in CapnpSplitter::run (splitter/capnp_splitter.rs:24-46).  Returns (d_offsets int64[n + 1] into d_bytes --
        message i = d_bytes[off[i]:off[i + 1]], its segment table included: with d_bytes what decode_frames_device(...,
        FG_FRAME_NONE) takes --, n, consumed, stop_reason (an FG_CAPNP_*)).  Nothing is packed and no UTF-8 pass runs.
        FgError(FG_ERR_UNSUPPORTED) when the device path declines the chunk: walk it on the host (CapnpFramer.frame).  d_bytes must
        start at a 16-byte aligned address and its memory must be readable up to numel() rounded up to 16."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        nbytes = d_bytes.numel()
        cap = cap_frames if cap_frames is not None else nbytes // 64 + 16
        while True:
            d_offsets = torch.empty(cap + 1, dtype=torch.int64, device=d_bytes.device)
            n, consumed, stop = C.c_uint64(), C.c_uint64(), C.c_int()
            rc = L.lib().fg_frame_capnp_device(self._ctx, d_bytes.data_ptr(), nbytes, int(final), d_offsets.data_ptr(), cap, C.byref(n),
                                               C.byref(consumed), C.byref(stop), C.c_void_p(stream.cuda_stream))
            if rc == L.FG_ERR_ENT_OVERFLOW and cap_frames is None:
                cap = int(n.value) + 16
                continue
            L.check(rc, "fg_frame_capnp_device")
            k = int(n.value)
            return d_offsets[:k + 1], k, int(consumed.value), int(stop.value)

    def last_capnp_stop(self) -> int:
        """how the chain of segment tables of the last FG_FRAME_CAPNP frame_decode_batch / Pipeline.run_stream on this decoder ended
        (FG_CAPNP_*)"""
        return int(L.lib().fg_last_capnp_stop(self._ctx))

    def last_host_path(self) -> int:
        """which form the last host-buffer call on this decoder took (FG_PATH_*)"""
        return int(L.lib().fg_last_host_path(self._ctx))

    def last_syslen_stop(self) -> int:
        """how the prefix chain of the last FG_FRAME_SYSLEN frame_decode_batch / Pipeline.run_stream on this decoder ended (FG_SYSLEN_*)"""
        return int(L.lib().fg_last_syslen_stop(self._ctx))

    def decode_frames_device(self, d_bytes, d_offsets, n: int, tables: DeviceTables, framing: int, d_bad=None,
                             stream=None) -> None:
        """Decode frames produced by frame_device (terminators are stripped inside the kernels; frames
        flagged in d_bad get status FG_ST_BAD_UTF8 = the reference's "Invalid UTF-8 input")."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        L.check(L.lib().fg_decode_frames_device(self._ctx, self.fmt, framing, d_bytes.data_ptr(), d_bytes.numel(),
                                                d_offsets.data_ptr(), n, d_bad.data_ptr() if d_bad is not None else None,
                                                C.byref(tables.struct), C.c_void_p(stream.cuda_stream)),
                "fg_decode_frames_device")

    def frame_decode_device(self, d_bytes, framing: int, tables: DeviceTables, cap_frames: int, final: bool = True, avg_line: int = 0,
                            stream=None):
        """Frame AND decode a raw byte stream resident in HBM in ONE kernel (fg_frame_decode_device: the decode kernels frame their
        tiles themselves; LineSplitter::run / NulSplitter::run for a chunk of the stream).  Asynchronous.  Returns
        (d_offsets int64[cap_frames + 2], d_result int64[2]): d_result[0] = frames found (rows beyond cap_frames were not written),
        d_result[1] != 0 = the launch gave up (use frame_device + decode_frames_device)."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        d_offsets = torch.empty(cap_frames + 2, dtype=torch.int64, device=d_bytes.device)
        d_result = torch.zeros(2, dtype=torch.int64, device=d_bytes.device)
        L.check(L.lib().fg_frame_decode_device(self._ctx, self.fmt, framing, d_bytes.data_ptr(), d_bytes.numel(), int(final),
                                               d_offsets.data_ptr(), cap_frames, C.byref(tables.struct), avg_line, d_result.data_ptr(),
                                               C.c_void_p(stream.cuda_stream)), "fg_frame_decode_device")
        return d_offsets, d_result

    def frame_decode_batch(self, raw: Union[bytes, np.ndarray], framing: int, final: bool = True):
        """Raw chunk of the byte stream in, tables out: GPU framing + UTF-8 validation + decode in one
        call (fg_frame_decode_batch; the body of LineSplitter::run / NulSplitter::run).  Returns
        (HostTables, offsets uint64[n+1], consumed): frame i = raw[offsets[i]:offsets[i+1]] including
        its terminator; raw[consumed:] is an unterminated tail to carry over (empty when `final`).
        framing = FG_FRAME_SYSLEN (the loop of SyslenSplitter::run): frame i starts with its "<len> " prefix and the tables' spans are
        relative to its payload; last_syslen_stop() says how the chain ended at `consumed`.
        framing = FG_FRAME_CAPNP (CapnpDecoder only; the read_message loop of CapnpSplitter::run): frame i is one whole message, its
        segment table included; last_capnp_stop() says how the chain ended at `consumed`."""
        buf = np.frombuffer(raw, np.uint8) if not isinstance(raw, np.ndarray) else np.ascontiguousarray(raw, np.uint8)
        padded = np.zeros(buf.size + 16, np.uint8)
        padded[:buf.size] = buf
        st = L.fg_tables()
        off = C.c_void_p()
        n, used = C.c_uint64(), C.c_uint64()
        L.check(L.lib().fg_frame_decode_batch(self._ctx, self.fmt, framing, padded.ctypes.data, buf.size, int(final),
                                              C.byref(st), C.byref(off), C.byref(n), C.byref(used)), "fg_frame_decode_batch")
        nf = int(n.value)
        if nf == 0:
            return None, np.zeros(1, np.uint64), int(used.value)
        offsets = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), (nf + 1,)).copy()
        return HostTables.from_struct(st), offsets, int(used.value)

    # -- the chunks of many connections in one launch ------------------------------------------------------
    def frame_multi_device(self, d_bytes, d_seg_starts, d_seg_final, framing: int, cap_slots: Optional[int] = None, stream=None):
        """fg_frame_multi_device: d_bytes holds the chunks of K connections back to back (segment k =
        d_bytes[seg_starts[k]:seg_starts[k + 1]], torch int64 / uint64 [K + 1]; d_seg_final uint8 [K] or None); every segment is
        framed as a stream of its own (`buf_reader.lines()` / `split(0)` + `str::from_utf8` per connection, tcp_input.rs:39-47).
        Returns (d_offsets, d_kind, n_slots, d_seg_first, d_seg_consumed): slot i = d_bytes[offsets[i]:offsets[i + 1]] including
        its terminator, kind FG_SLOT_FRAME / _BAD_UTF8 / _CARRY; d_kind is decode_frames_device's d_bad as it is."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        nbytes, K = d_bytes.numel(), d_seg_starts.numel() - 1
        cap = cap_slots if cap_slots is not None else nbytes // 16 + K + 16
        d_first = torch.empty(K + 1, dtype=torch.int64, device=d_bytes.device)
        d_cons = torch.empty(max(K, 1), dtype=torch.int64, device=d_bytes.device)

        def attempt(cap):
            d_offsets = torch.empty(cap + 1, dtype=torch.int64, device=d_bytes.device)
            d_kind = torch.empty(max(cap, 1), dtype=torch.uint8, device=d_bytes.device)
            n = C.c_uint64()
            rc = L.lib().fg_frame_multi_device(self._ctx, framing, d_bytes.data_ptr(), nbytes, d_seg_starts.data_ptr(),
                                               d_seg_final.data_ptr() if d_seg_final is not None else None, K, d_offsets.data_ptr(),
                                               d_kind.data_ptr(), cap, d_first.data_ptr(), d_cons.data_ptr(), C.byref(n),
                                               C.c_void_p(stream.cuda_stream))
            return rc, int(n.value), (d_offsets, d_kind)

        n, (d_offsets, d_kind) = _framed_within("fg_frame_multi_device", cap, cap_slots is not None, 0, attempt)
        return d_offsets, d_kind, n, d_first, d_cons[:K]

    def frame_decode_multi(self, raw: Union[bytes, np.ndarray], seg_starts, seg_final, framing: int):
        """fg_frame_decode_multi_batch: the chunks of K connections back to back in, tables out.  Returns (HostTables or None, offsets
        uint64[n + 1], kind uint8[n], seg_first uint64[K + 1], seg_consumed uint64[K]); rows of FG_SLOT_BAD_UTF8 and FG_SLOT_CARRY slots
        have status FG_ST_BAD_UTF8."""
        buf = np.frombuffer(raw, np.uint8) if not isinstance(raw, np.ndarray) else np.ascontiguousarray(raw, np.uint8)
        starts = np.ascontiguousarray(seg_starts, np.uint64)
        K = len(starts) - 1
        final = None if seg_final is None else np.ascontiguousarray(seg_final, np.uint8)
        st = L.fg_tables()
        off, kind, first, cons = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = C.c_uint64()
        L.check(L.lib().fg_frame_decode_multi_batch(self._ctx, self.fmt, framing, buf.ctypes.data if buf.size else None, buf.size,
                                                    starts.ctypes.data, final.ctypes.data if final is not None and K else None, K,
                                                    C.byref(st), C.byref(off), C.byref(kind), C.byref(first), C.byref(cons), C.byref(n)),
                "fg_frame_decode_multi_batch")
        ns = int(n.value)
        return ((HostTables.from_struct(st) if ns else None), _copied(off, C.c_uint64, ns + 1), _copied(kind, C.c_uint8, ns),
                _copied(first, C.c_uint64, K + 1), _copied(cons, C.c_uint64, K))

    def frame_syslen_multi_device(self, d_bytes, d_seg_starts, cap_frames: Optional[int] = None, stream=None):
        """fg_frame_syslen_multi_device: d_bytes holds the octet-counted chunks of K connections back to back (segment k =
        d_bytes[seg_starts[k]:seg_starts[k + 1]], torch int64 / uint64 [K + 1]); every segment is walked as a stream of its own (a
        SyslenSplitter per connection, tcp_input.rs:39-47), FRAMED AND PACKED in buffer order.  Returns (d_packed uint8, d_offsets
        int64[n + 1] into d_packed, d_frame_starts int64[n] into d_bytes, d_bad uint8[n], n, d_seg_first int64[K + 1], d_seg_consumed
        int64[K], d_seg_stop uint8[K] (FG_SYSLEN_*), payload_bytes).  FgError(FG_ERR_UNSUPPORTED) when the device path declines the
        buffer: frame it on the host.  d_bytes as frame_syslen_device wants it."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        dev = d_bytes.device
        nbytes, K = d_bytes.numel(), d_seg_starts.numel() - 1
        cap = cap_frames if cap_frames is not None else nbytes // 32 + 16
        d_packed = torch.empty((nbytes + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
        d_first = torch.empty(K + 1, dtype=torch.int64, device=dev)
        d_cons = torch.empty(max(K, 1), dtype=torch.int64, device=dev)
        d_stop = torch.empty(max(K, 1), dtype=torch.uint8, device=dev)

        def attempt(cap):
            d_offsets = torch.empty(cap + 1, dtype=torch.int64, device=dev)
            d_starts = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
            d_bad = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            n, payload = C.c_uint64(), C.c_uint64()
            rc = L.lib().fg_frame_syslen_multi_device(self._ctx, d_bytes.data_ptr(), nbytes, d_seg_starts.data_ptr(), K, d_packed.data_ptr(),
                                                      d_offsets.data_ptr(), d_starts.data_ptr(), d_bad.data_ptr(), cap, d_first.data_ptr(),
                                                      d_cons.data_ptr(), d_stop.data_ptr(), C.byref(n), C.byref(payload),
                                                      C.c_void_p(stream.cuda_stream))
            return rc, int(n.value), (d_offsets, d_starts, d_bad, int(payload.value))

        k, (d_offsets, d_starts, d_bad, payload) = _framed_within("fg_frame_syslen_multi_device", cap, cap_frames is not None, 16, attempt)
        return d_packed, d_offsets[:k + 1], d_starts[:k], d_bad[:k], k, d_first, d_cons[:K], d_stop[:K], payload

    def frame_decode_syslen_multi(self, raw: Union[bytes, np.ndarray], seg_starts):
        """fg_frame_decode_syslen_multi_batch: the octet-counted chunks of K connections back to back in, tables out.  Returns
        (HostTables or None, frame_starts uint64[n], seg_first uint64[K + 1], seg_consumed uint64[K], seg_stop uint8[K]); frame i
        starts with its "<len> " prefix at raw[frame_starts[i]], the tables' spans are relative to its payload, and a payload that is
        not valid UTF-8 has status FG_ST_BAD_UTF8.  last_host_path() says whether the device framed the buffer or the host hopped it."""
        buf = np.frombuffer(raw, np.uint8) if not isinstance(raw, np.ndarray) else np.ascontiguousarray(raw, np.uint8)
        starts = np.ascontiguousarray(seg_starts, np.uint64)
        K = len(starts) - 1
        st = L.fg_tables()
        fs, first, cons, stop = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = C.c_uint64()
        L.check(L.lib().fg_frame_decode_syslen_multi_batch(self._ctx, self.fmt, buf.ctypes.data if buf.size else None, buf.size,
                                                           starts.ctypes.data, K, C.byref(st), C.byref(fs), C.byref(first), C.byref(cons),
                                                           C.byref(stop), C.byref(n)), "fg_frame_decode_syslen_multi_batch")
        nf = int(n.value)
        return ((HostTables.from_struct(st) if nf else None), _copied(fs, C.c_uint64, nf), _copied(first, C.c_uint64, K + 1),
                _copied(cons, C.c_uint64, K), _copied(stop, C.c_uint8, K))

    def frame_capnp_multi_device(self, d_bytes, d_seg_starts, cap_slots: Optional[int] = None, stream=None):
        """fg_frame_capnp_multi_device: d_bytes holds the Cap'n Proto chunks of K connections back to back (segment k =
        d_bytes[seg_starts[k]:seg_starts[k + 1]], torch int64 / uint64 [K + 1], every start but the last a multiple of 8); every
        segment is walked as a stream of its own (a CapnpSplitter per connection, tcp_input.rs:39-47).  Returns (d_offsets int64[n + 1],
        d_kind uint8[n], n_slots, d_seg_first int64[K + 1], d_seg_consumed int64[K], d_seg_stop uint8[K] (FG_CAPNP_*)): slot i =
        d_bytes[offsets[i]:offsets[i + 1]], kind FG_SLOT_FRAME (a whole message) or FG_SLOT_CARRY (the bytes of a segment behind its
        consumed); d_kind is decode_frames_device's d_bad as it is.  FgError(FG_ERR_UNSUPPORTED) when the device path declines the
        buffer: walk it on the host.  d_bytes as frame_capnp_device wants it."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        dev = d_bytes.device
        nbytes, K = d_bytes.numel(), d_seg_starts.numel() - 1
        cap = cap_slots if cap_slots is not None else nbytes // 64 + K + 16
        d_first = torch.empty(K + 1, dtype=torch.int64, device=dev)
        d_cons = torch.empty(max(K, 1), dtype=torch.int64, device=dev)
        d_stop = torch.empty(max(K, 1), dtype=torch.uint8, device=dev)

        def attempt(cap):
            d_offsets = torch.empty(cap + 1, dtype=torch.int64, device=dev)
            d_kind = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            n = C.c_uint64()
            rc = L.lib().fg_frame_capnp_multi_device(self._ctx, d_bytes.data_ptr(), nbytes, d_seg_starts.data_ptr(), K, d_offsets.data_ptr(),
                                                     d_kind.data_ptr(), cap, d_first.data_ptr(), d_cons.data_ptr(), d_stop.data_ptr(),
                                                     C.byref(n), C.c_void_p(stream.cuda_stream))
            return rc, int(n.value), (d_offsets, d_kind)

        k, (d_offsets, d_kind) = _framed_within("fg_frame_capnp_multi_device", cap, cap_slots is not None, 16, attempt)
        return d_offsets[:k + 1], d_kind[:k], k, d_first, d_cons[:K], d_stop[:K]

    def frame_decode_capnp_multi(self, raw: Union[bytes, np.ndarray], seg_starts):
        """fg_frame_decode_capnp_multi_batch: the Cap'n Proto chunks of K connections back to back in, tables out.  Returns (HostTables
        or None, offsets uint64[n + 1], kind uint8[n], seg_first uint64[K + 1], seg_consumed uint64[K], seg_stop uint8[K]); the row of
        a FG_SLOT_CARRY slot has status FG_ST_BAD_UTF8.  last_host_path() says whether the device framed the buffer or the host
        walked it."""
        buf = np.frombuffer(raw, np.uint8) if not isinstance(raw, np.ndarray) else np.ascontiguousarray(raw, np.uint8)
        starts = np.ascontiguousarray(seg_starts, np.uint64)
        K = len(starts) - 1
        st = L.fg_tables()
        off, kind, first, cons, stop = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = C.c_uint64()
        L.check(L.lib().fg_frame_decode_capnp_multi_batch(self._ctx, buf.ctypes.data if buf.size else None, buf.size, starts.ctypes.data, K,
                                                          C.byref(st), C.byref(off), C.byref(kind), C.byref(first), C.byref(cons),
                                                          C.byref(stop), C.byref(n)), "fg_frame_decode_capnp_multi_batch")
        ns = int(n.value)
        return ((HostTables.from_struct(st) if ns else None), _copied(off, C.c_uint64, ns + 1), _copied(kind, C.c_uint8, ns),
                _copied(first, C.c_uint64, K + 1), _copied(cons, C.c_uint64, K), _copied(stop, C.c_uint8, K))

    # -- the UDP input (input/udp_input.rs:100-143) -------------------------------------------------------
    def udp_decode_packed(self, data: np.ndarray, offsets: np.ndarray, max_inflated: Optional[int] = None):
        """Datagrams back to back in, tables out (fg_udp_decode_batch: upload, inflate / copy + UTF-8 on the GPU, decode).  Returns
        (HostTables, lines uint8, line_offsets uint64[n + 1], udp_status uint8[n]): the tables' spans are relative to the INFLATED
        line i = lines[line_offsets[i]:line_offsets[i + 1]]; a dropped datagram has status FG_ST_BAD_UTF8 and its FG_UDP_* reason in
        udp_status."""
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        st = L.fg_tables()
        lines, offs, ust = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(L.lib().fg_udp_decode_batch(self._ctx, self.fmt, data.ctypes.data, data.size, offsets.ctypes.data, n, int(max_inflated or 0),
                                            C.byref(st), C.byref(lines), C.byref(offs), C.byref(ust)), "fg_udp_decode_batch")
        if n == 0:
            return None, np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint8)
        line_offsets = np.ctypeslib.as_array(C.cast(offs, C.POINTER(C.c_uint64)), (n + 1,)).copy()
        total = int(line_offsets[n])
        out = np.zeros(total + 16, np.uint8)  # (the pad the host-side readers of a batch expect)
        if total:
            out[:total] = np.ctypeslib.as_array(C.cast(lines, C.POINTER(C.c_uint8)), (total,))
        status = np.ctypeslib.as_array(C.cast(ust, C.POINTER(C.c_uint8)), (n,)).copy()
        return HostTables.from_struct(st), out[:total], line_offsets, status

    def decode_datagrams(self, datagrams: Sequence[bytes], max_inflated: Optional[int] = None) -> List[Union[Record, DecodeError]]:
        """handle_record_maybe_compressed (input/udp_input.rs:100-143) for a list of UDP datagrams: each is a zlib stream, a gzip
        member or a bare record; a Record or the DecodeError the reference prints per datagram ("Corrupted compressed (zlib) record",
        "Corrupted compressed (gzip) record", "Invalid UTF-8 input", or the decoder's own).  max_inflated: the most a compressed
        datagram may inflate to (None = 65 527 * 5); one beyond it is a DecodeError of this library's own -- inflate it on the host."""
        data, offsets = pack_lines(datagrams)
        if len(datagrams) == 0:
            return []
        tab, lines, line_offsets, ust = self.udp_decode_packed(data, offsets, max_inflated)
        blob, offs = tab.serialize(self.fmt, lines, line_offsets, cfg=self._cfg)
        raw = blob.tobytes()
        out: List[Union[Record, DecodeError]] = []
        for i in range(len(datagrams)):
            if ust[i] > L.FG_UDP_GZIP:
                out.append(DecodeError(L.lib().fg_udp_error_string(int(ust[i])).decode()))
            else:
                out.append(parse_canonical(raw[int(offs[i]):int(offs[i + 1])]))
        return out

    # -- GELF encoder from the tables ------------------------------------------------
    def encode_gelf_device(self, d_bytes, d_offsets, n: int, tables: DeviceTables, extra: Optional[dict] = None, stream=None):
        """GelfEncoder::encode (encoder/gelf_encoder.rs:59-115) for every decoded line of `tables`, on the
        GPU, without materialising Records.  `extra` = the output.gelf_extra table.  Returns
        (d_out uint8, d_out_offsets int64[n+1]): JSON of line i = d_out[off[i]:off[i+1]] (empty for a
        line whose decode failed)."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        items = list((extra or {}).items())
        ks = (C.c_char_p * max(len(items), 1))(*[k.encode() for k, _ in items])
        vs = (C.c_char_p * max(len(items), 1))(*[v.encode() for _, v in items])
        ex = L.fg_gelf_extra(len(items), C.cast(ks, C.POINTER(C.c_char_p)), C.cast(vs, C.POINTER(C.c_char_p)))
        d_off = torch.empty(n + 1, dtype=torch.int64, device=d_bytes.device)
        total = C.c_uint64()
        args = (self._ctx, self.fmt, d_bytes.data_ptr(), d_bytes.numel(), d_offsets.data_ptr(), n, C.byref(tables.struct), C.byref(ex))
        L.check(L.lib().fg_encode_gelf_device(*args, None, 0, d_off.data_ptr(), C.byref(total), C.c_void_p(stream.cuda_stream)),
                "fg_encode_gelf_device (size)")
        d_out = torch.empty(max(int(total.value), 1), dtype=torch.uint8, device=d_bytes.device)
        L.check(L.lib().fg_encode_gelf_device(*args, d_out.data_ptr(), d_out.numel(), d_off.data_ptr(), C.byref(total),
                                              C.c_void_p(stream.cuda_stream)), "fg_encode_gelf_device")
        return d_out[:int(total.value)], d_off

    def set_timing(self, enabled: bool = True) -> None:
        L.check(L.lib().fg_set_timing(self._ctx, int(enabled)), "fg_set_timing")

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        L.check(L.lib().fg_last_kernel_ms(self._ctx, C.byref(ms)), "fg_last_kernel_ms")
        return float(ms.value)

    def error_string(self, status: int) -> Optional[str]:
        s = L.lib().fg_error_string(self.fmt, status)
        return None if s is None else s.decode()


class UdpUnpacker:
    """The device-resident form of the UDP input's body (fg_udp_unpack_device): datagrams in HBM in, the payloads -- inflated where
    they were compressed, UTF-8 checked -- packed in HBM out, ready for Decoder.decode_frames_device(..., FG_FRAME_NONE, d_bad=d_drop)."""

    def __init__(self, decoder: Decoder, max_inflated: Optional[int] = None):
        self.decoder = decoder
        self.max_inflated = int(max_inflated or 0)

    def unpack(self, d_bytes, d_offsets, stream=None):
        """d_bytes uint8, d_offsets int64[n + 1] (torch tensors in HBM) -> (d_out uint8, d_out_offsets int64[n + 1], d_drop uint8[n],
        d_udp_status uint8[n]).  Synchronises the stream twice (the size, then the result)."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        n = d_offsets.numel() - 1
        dev = d_bytes.device
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_drop = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        d_st = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        total = C.c_uint64()
        args = (self.decoder._ctx, d_bytes.data_ptr(), d_bytes.numel(), d_offsets.data_ptr(), n, self.max_inflated)
        tail = (d_off.data_ptr(), d_drop.data_ptr(), d_st.data_ptr(), C.byref(total), C.c_void_p(stream.cuda_stream))
        L.check(L.lib().fg_udp_unpack_device(*args, None, 0, *tail), "fg_udp_unpack_device (size)")
        cap = int(total.value)
        d_out = torch.zeros((cap + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
        L.check(L.lib().fg_udp_unpack_device(*args, d_out.data_ptr(), cap, *tail), "fg_udp_unpack_device")
        return d_out[:cap], d_off, d_drop[:n], d_st[:n]

    def unpack_once(self, d_bytes, d_offsets, stream=None, out_cap=None):
        """The same results from ONE walk per stream (fg_udp_unpack_once_device).  There is no sizing call, so the output buffer is a
        guess: out_cap bytes (None: twice the datagrams' bytes + 4 KiB).  When the batch needs more the call says how much and is
        made again with a buffer of that size (a host that never wants the walk twice uses Pipeline.run_datagrams, which sizes its
        buffer between the walk and the pack).  `.last_spilled()`: how many streams outgrew their stage and were written by a
        second walk.  The stream is synchronised before the tensors are returned."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        n = d_offsets.numel() - 1
        dev = d_bytes.device
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_drop = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        d_st = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        total = C.c_uint64()
        args = (self.decoder._ctx, d_bytes.data_ptr(), d_bytes.numel(), d_offsets.data_ptr(), n, self.max_inflated)
        tail = (d_off.data_ptr(), d_drop.data_ptr(), d_st.data_ptr(), C.byref(total), C.c_void_p(stream.cuda_stream))
        cap = int(2 * d_bytes.numel() + 4096 if out_cap is None else out_cap)
        d_out = torch.zeros((cap + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
        rc = L.lib().fg_udp_unpack_once_device(*args, d_out.data_ptr(), cap, *tail)
        if rc == L.FG_ERR_ENT_OVERFLOW:
            cap = int(total.value)
            d_out = torch.zeros((cap + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
            rc = L.lib().fg_udp_unpack_once_device(*args, d_out.data_ptr(), cap, *tail)
        L.check(rc, "fg_udp_unpack_once_device")
        stream.synchronize()
        cap = int(total.value)
        return d_out[:cap], d_off, d_drop[:n], d_st[:n]

    def last_spilled(self) -> int:
        return int(L.lib().fg_udp_last_spilled(self.decoder._ctx))


class FlushPolicy:
    """When a batching framer hands what it holds to the GPU (the fields of the C++ fg::FlushPolicy that make sense before the lines
    are counted): max_bytes -- a batch never grows beyond this; max_latency_ms -- how long the first chunk of a batch may wait for
    company."""

    def __init__(self, max_bytes: int = 8 << 20, max_latency_ms: float = 5.0):
        self.max_bytes, self.max_latency_ms = max_bytes, max_latency_ms


_RUST_WS = "\t\n\x0b\x0c\r \x85\xa0\u1680\u2000\u2001\u2002\u2003\u2004\u2005\u2006\u2007\u2008\u2009\u200a\u2028\u2029\u202f\u205f\u3000"


class _MultiSplitter:
    """What the multi-connection splitters share: the chunks of many connections parked until the policy says the batch is due, and
    the bytes each connection carries over from its last batch.  A subclass frames and decodes what _take() hands it in flush()."""

    PUSH_REFUSED = "push after the connection ended"

    def __init__(self, decoder: Decoder, policy: Optional[FlushPolicy] = None):
        self.decoder, self.policy = decoder, policy or FlushPolicy()
        self._carry: dict = {}     # conn -> bytes carried over from its last flushed chunk
        self._pending: dict = {}   # conn -> chunks pushed since the last flush (insertion order = arrival order)
        self._closed: set = set()  # close() seen, not flushed yet
        self._bytes = 0
        self._first_at: Optional[float] = None

    def _ended(self, conn_id) -> bool:
        """the connection is over for good: it may not push, and closing it again means nothing"""
        return False

    @staticmethod
    def _trimmed(frame: bytes) -> str:
        """str::trim of a frame: what the reference prints between the brackets of its stderr line"""
        return frame.decode("utf-8").strip(_RUST_WS)

    @staticmethod
    def _unterminated(line: bytes, framing: int) -> bytes:
        """a LINE / NUL slot without its terminator ("\n" or "\r\n": BufRead::lines; the NUL)"""
        if framing == L.FG_FRAME_LINE:
            return line[:-2] if line.endswith(b"\r\n") else line[:-1] if line.endswith(b"\n") else line
        return line[:-1] if line.endswith(b"\0") else line

    def _decode_error(self, r, frame: bytes) -> DecodeError:
        """"<the decoder's or the encoder's error>: [<trimmed frame>]" (line_splitter.rs:37-39, syslen_splitter.rs:35-37)"""
        return DecodeError(f"{r}: [{self._trimmed(frame)}]")

    def push(self, conn_id, chunk: bytes) -> list:
        """park a chunk; -> flush()'s result when the policy says the batch is due, else []"""
        import time

        if conn_id in self._closed or self._ended(conn_id):
            raise ValueError(self.PUSH_REFUSED)
        if chunk:
            self._pending.setdefault(conn_id, []).append(bytes(chunk))
            self._bytes += len(chunk)
            if self._first_at is None:
                self._first_at = time.monotonic()
        due = self._bytes >= self.policy.max_bytes or (
            self._first_at is not None and (time.monotonic() - self._first_at) * 1e3 >= self.policy.max_latency_ms)
        return self.flush() if due else []

    def close(self, conn_id) -> None:
        """the connection's EOF, acted on at the next flush (the class says how)"""
        if not self._ended(conn_id):
            self._closed.add(conn_id)
            self._pending.setdefault(conn_id, [])

    def pending_bytes(self) -> int:
        return self._bytes

    def _take(self, align: int = 1):
        """-> (conns in arrival order, what each holds: carry + parked chunks, raw, starts uint64[K + 1]) and resets the batch; raw holds
        the first len - len % align bytes of every connection back to back, connection k at raw[starts[k]:starts[k + 1]]"""
        conns = list(self._pending)
        segs = [self._carry.pop(c, b"") + b"".join(self._pending[c]) for c in conns]
        self._pending, self._bytes, self._first_at = {}, 0, None
        sent = [s[:len(s) - len(s) % align] for s in segs]
        starts = np.zeros(len(segs) + 1, np.uint64)
        starts[1:] = np.cumsum([len(s) for s in sent], dtype=np.uint64)
        return conns, segs, b"".join(sent), starts


class _EndingSplitter(_MultiSplitter):
    """... whose connections can end for good (their EOF, or input that ends them): _over"""

    def __init__(self, decoder: Decoder, policy: Optional[FlushPolicy] = None):
        super().__init__(decoder, policy)
        self._over: set = set()

    def _ended(self, conn_id) -> bool:
        return conn_id in self._over

    def _empty_message(self) -> list:
        """what handling an empty octet-counted message yields"""
        r = self.decoder.decode_batch([b""])[0]
        return [self._decode_error(r, b"") if isinstance(r, DecodeError) else r]

    def _eof(self, tail: bytes) -> list:
        """what SyslenSplitter::run reports when the stream ends with `tail` behind the last whole frame (fg_decoder.hpp's Syslen
        branch: read_until drops the last byte of a length that no ' ' follows)"""
        sp = tail.find(b" ")
        if sp >= 0:  # a whole prefix (a bad one ended the connection before): EOF inside its payload
            return [DecodeError(SYSLEN_SHORT_READ)]
        num = tail[:-1]
        body = num[1:] if num[:1] == b"+" else num
        if len(tail) <= 1 or not body or not body.isdigit() or int(body) >= 1 << 64:
            return [DecodeError(SYSLEN_BAD_LENGTH)]
        if int(body) != 0:
            return [DecodeError(SYSLEN_SHORT_READ)]
        # "0?" + EOF: an empty message is handled, then the next read_msglen sees Ok(0)
        return self._empty_message() + [DecodeError(SYSLEN_BAD_LENGTH)]


class MultiStreamSplitter(_MultiSplitter):
    """The stream-side sibling of the UDP batcher: parks the chunks of MANY connections and hands them to the GPU together -- one
    fg_frame_decode_multi_batch call frames every connection's bytes as its own stream and decodes the frames.  Per connection the
    output is what LineSplitter::run / NulSplitter::run (splitter/line_splitter.rs:17-54, nul_splitter.rs:18-60) produce for the bytes
    pushed so far: a Record per decoded line, or a DecodeError whose text is the reference's stderr line -- "Invalid UTF-8 input", or
    "<decoder's error>: [<trimmed line>]" (NUL framing prints nothing for a frame that trims to nothing, nul_splitter.rs:41-46).
    The unterminated tail of a connection's chunk is carried over and prepended to its next one; close(conn) is its EOF."""

    PUSH_REFUSED = "push after close"  # (a closed connection is forgotten at the next flush: its id may come back)

    def __init__(self, decoder: Decoder, framing: int, policy: Optional[FlushPolicy] = None):
        if framing not in (L.FG_FRAME_LINE, L.FG_FRAME_NUL):
            raise ValueError("MultiStreamSplitter frames FG_FRAME_LINE or FG_FRAME_NUL streams")
        super().__init__(decoder, policy)
        self.framing = framing

    def flush(self) -> list:
        """-> [(conn_id, [Record | DecodeError, ...]), ...] for every connection that had chunks parked or was closed, in arrival order"""
        conns, _, raw, starts = self._take()
        final = [1 if c in self._closed else 0 for c in conns]  # (close(conn): its unterminated tail is a frame)
        self._closed.difference_update(conns)
        if not conns:
            return []
        tab, offsets, kind, first, _ = self.decoder.frame_decode_multi(raw, starts, final, self.framing)
        out = []
        can, coffs = b"", None
        if tab is not None:
            can, coffs = self.decoder._canonical(tab, np.frombuffer(raw + b"\0" * 32, np.uint8), offsets, self.framing)
        for k, c in enumerate(conns):
            res: list = []
            for i in range(int(first[k]), int(first[k + 1])):
                a, b = int(offsets[i]), int(offsets[i + 1])
                if kind[i] == L.FG_SLOT_CARRY:
                    self._carry[c] = raw[a:b]
                elif kind[i] == L.FG_SLOT_BAD_UTF8:
                    res.append(DecodeError("Invalid UTF-8 input"))
                else:
                    r = parse_canonical(can[int(coffs[i]):int(coffs[i + 1])])
                    if isinstance(r, DecodeError):
                        line = self._unterminated(raw[a:b], self.framing)
                        if self.framing == L.FG_FRAME_NUL and not self._trimmed(line):
                            continue
                        r = self._decode_error(r, line)
                    res.append(r)
            out.append((c, res))
        return out


SYSLEN_BAD_LENGTH = "Can't read message's length"                       # syslen_splitter.rs:45-46
SYSLEN_SHORT_READ = "failed to fill whole buffer"                        # read_exact's UnexpectedEof, printed with `{}` (:27-30)
SYSLEN_PANIC = "thread panicked: called `Result::unwrap()` on an `Err` value: FromUtf8Error (syslen_splitter.rs:32)"


class MultiSyslenSplitter(_EndingSplitter):
    """MultiStreamSplitter for OCTET-COUNTED connections (input.framing = "syslen": tcpco / tlsco inputs): parks the chunks of many
    connections and hands them to the GPU together -- one fg_frame_decode_syslen_multi_batch call walks every connection's bytes as its
    own stream and decodes the payloads.  Per connection the output is what SyslenSplitter::run (splitter/syslen_splitter.rs:17-57)
    produces for the bytes pushed so far: a Record per frame that decodes, DecodeError("<decoder's error>: [<trimmed payload>]") per
    frame that does not; the bytes behind the last whole frame are carried over to the connection's next chunk.  A length that cannot
    be read ends the connection with DecodeError("Can't read message's length"), the first payload that is not valid UTF-8 with the
    reference's panic text (its `unwrap()`): later pushes raise.  close(conn) is its EOF: "Can't read message's length" with nothing
    carried, else what the reference reports for an EOF inside a length or a payload."""

    def flush(self) -> list:
        """-> [(conn_id, [Record | DecodeError, ...]), ...] for every connection that had chunks parked or was closed, in arrival order"""
        conns, segs, raw, starts = self._take()
        if not conns:
            return []
        tab, fstart, first, cons, stop = self.decoder.frame_decode_syslen_multi(raw, starts)
        payloads = []
        for a in fstart:
            sp = raw.index(b" ", int(a))
            payloads.append(raw[sp + 1:sp + 1 + int(raw[int(a):sp])])
        can, coffs = b"", None
        if tab is not None:
            data, offsets = pack_lines(payloads)
            can, coffs = self.decoder._canonical(tab, np.concatenate([data, np.zeros(32, np.uint8)]), offsets)
            status = tab.a["meta"][:tab.n] & 0xFF
        out = []
        for k, c in enumerate(conns):
            res: list = []
            over = False
            for i in range(int(first[k]), int(first[k + 1])):
                if status[i] == L.FG_ST_BAD_UTF8:  # the reference's unwrap(): this connection's thread ends here
                    res.append(DecodeError(SYSLEN_PANIC))
                    over = True
                    break
                r = parse_canonical(can[int(coffs[i]):int(coffs[i + 1])])
                res.append(self._decode_error(r, payloads[i]) if isinstance(r, DecodeError) else r)
            if not over and stop[k] == L.FG_SYSLEN_BAD_LEN:
                res.append(DecodeError(SYSLEN_BAD_LENGTH))
                over = True
            tail = segs[k][int(cons[k]):]
            if not over and c in self._closed:
                res += self._eof(tail) if tail else [DecodeError(SYSLEN_BAD_LENGTH)]
                over = True
            self._closed.discard(c)
            if over:
                self._over.add(c)
            elif tail:
                self._carry[c] = tail
            out.append((c, res))
        return out


class RFC5424Decoder(Decoder):
    """src/flowgger/decoder/rfc5424_decoder.rs:8-50 (stateless; config ignored, :12-14)."""
    fmt = L.FG_RFC5424


class GelfDecoder(Decoder):
    """src/flowgger/decoder/gelf_decoder.rs:10-125 (config ignored, :16-18)."""
    fmt = L.FG_GELF


def pack_messages(messages: Iterable[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """The container of an FG_CAPNP batch: whole Cap'n Proto messages (segment table included) -> (packed bytes, offsets[n+1]).
    A message is an array of 8-byte words and starts on one (include/fg_hip.h): a message whose length is no whole number of words
    is refused (ValueError), as the C ABI refuses offsets that are no multiples of 8."""
    bl = [bytes(m) for m in messages]
    for i, b in enumerate(bl):
        if len(b) & 7:
            raise ValueError(f"message {i}: {len(b)} bytes is not a whole number of 8-byte words")
    offsets = np.zeros(len(bl) + 1, np.uint64)
    if bl:
        offsets[1:] = np.cumsum([len(b) for b in bl], dtype=np.uint64)
    data = np.frombuffer(b"".join(bl), np.uint8).copy() if bl else np.zeros(0, np.uint8)
    return data, offsets


class CapnpStreamError(Exception):
    """capnp::serialize::read_message failed: the reference prints "Capnp decoding error: ..." and ends the connection
    (splitter/capnp_splitter.rs:26-31).  `offsets` / `consumed`: the whole messages in front of the bad table, which the reference
    has handled by then."""

    def __init__(self, text: str, offsets=None, consumed: int = 0):
        super().__init__(text)
        self.offsets = np.zeros(1, np.uint64) if offsets is None else offsets
        self.consumed = consumed


class CapnpFramer:
    """The framing half of CapnpSplitter::run (splitter/capnp_splitter.rs:24-46): a Cap'n Proto stream is a chain of length
    prefixes -- message k + 1 starts where the segment table of message k says -- so the walk stays on the host and reads one
    table per message.  ``feed(chunk)`` returns the whole messages now available as (packed bytes, offsets) for
    :meth:`CapnpDecoder.decode_packed`; an incomplete last message is carried over to the next call.  The two conditions under
    which capnp 0.14's ``read_message`` (default ``ReaderOptions``) ends the connection raise :class:`CapnpStreamError`:
    512 or more segments, more than 8 Mi words in total."""

    MAX_SEGMENTS = 512
    MAX_WORDS = 8 << 20

    def __init__(self):
        self._carry = b""
        self._ended = None  # the CapnpStreamError that ended the connection

    @classmethod
    def frame(cls, buf: Union[bytes, memoryview]) -> Tuple[np.ndarray, int]:
        """(offsets of the whole messages at the front of `buf`, bytes they cover)"""
        import struct

        mv = memoryview(buf)
        offs, p, n_buf = [0], 0, len(mv)
        while n_buf - p >= 8:
            n = struct.unpack_from("<I", mv, p)[0] + 1
            if n >= cls.MAX_SEGMENTS:
                raise CapnpStreamError(f"Too many segments: {n}", np.array(offs, np.uint64), p)
            table = (4 + 4 * n + 7) // 8 * 8
            if n_buf - p < table:
                break
            words = sum(struct.unpack_from(f"<{n}I", mv, p + 4))
            if words > cls.MAX_WORDS:
                raise CapnpStreamError(f"Message has {words} words, which is too large", np.array(offs, np.uint64), p)
            if n_buf - p < table + 8 * words:
                break
            p += table + 8 * words
            offs.append(p)
        return np.array(offs, np.uint64), p

    def feed(self, chunk: bytes) -> Tuple[np.ndarray, np.ndarray]:
        if self._ended is not None:
            raise self._ended
        buf = self._carry + bytes(chunk)
        try:
            offsets, consumed = self.frame(buf)
        except CapnpStreamError as e:
            # the whole messages in front of the bad table are handled first (capnp_splitter.rs:24-60): they are returned now and
            # the error is raised by the next call -- at once when there are none
            self._ended = e
            if len(e.offsets) < 2:
                raise
            offsets, consumed = e.offsets, e.consumed
        self._carry = buf[consumed:]
        return np.frombuffer(buf[:consumed], np.uint8).copy(), offsets

    @property
    def pending(self) -> int:
        """bytes of an incomplete message carried over"""
        return len(self._carry)


class _GpuCapnpCarry:
    """The carry-over of the gpu_framing routes of CapnpSplitter / CapnpTranscodingSplitter: what CapnpFramer.feed does around the walk,
    around FG_FRAME_CAPNP calls instead.  The tail behind `consumed` is kept for the next chunk; a table that ends the connection
    raises the CapnpStreamError CapnpFramer would -- after the whole messages in front of it have been returned, at once when there
    are none."""

    def __init__(self):
        self._carry = b""
        self._ended = None

    def begin(self, chunk: bytes) -> bytes:
        if self._ended is not None:
            raise self._ended
        return self._carry + bytes(chunk)

    def end(self, buf: bytes, n: int, consumed: int, stop: int) -> None:
        self._carry = buf[consumed:]
        if stop in (L.FG_CAPNP_TOO_MANY_SEGMENTS, L.FG_CAPNP_TOO_LARGE):
            try:
                CapnpFramer.frame(self._carry)  # (the text of the error: the few words of the table at `consumed`)
                raise AssertionError("the device framer stopped at a table the host walk accepts")
            except CapnpStreamError as e:
                self._ended = e
            if n == 0:
                raise self._ended

    @property
    def pending(self) -> int:
        return len(self._carry)


class CapnpDecoder(Decoder):
    """handle_message of src/flowgger/splitter/capnp_splitter.rs:65-167 (input.format = "capnp"; the reference has no Decoder for
    it: the splitter reads Records off the wire itself).  A "line" is one whole message, segment table included."""
    fmt = L.FG_CAPNP

    def decode_batch(self, lines: Sequence[bytes]) -> List[Union[Record, DecodeError]]:
        data, offsets = pack_messages(lines)
        tab = self.decode_packed(data, offsets)
        blob, offs = tab.serialize(self.fmt, data, offsets)
        raw = blob.tobytes()
        return [parse_canonical(raw[int(offs[i]):int(offs[i + 1])]) for i in range(len(lines))]


class CapnpSplitter:
    """CapnpSplitter::run (splitter/capnp_splitter.rs:15-63) without the encoder: chunks of the stream in, Records (or the
    DecodeError the reference prints) out, in stream order."""

    def __init__(self, decoder: Optional[CapnpDecoder] = None, device: int = 0, gpu_framing: bool = False):
        """gpu_framing: the chunk (behind the tail carried over) goes to the GPU as it is and is framed there (FG_FRAME_CAPNP); the
        Records, the carry-over and the CapnpStreamError are the host-framed route's."""
        self.decoder = decoder or CapnpDecoder(device=device)
        self.framer = _GpuCapnpCarry() if gpu_framing else CapnpFramer()
        self.gpu_framing = gpu_framing

    def feed(self, chunk: bytes) -> List[Union[Record, DecodeError]]:
        if self.gpu_framing:
            buf = self.framer.begin(chunk)
            tab, offsets, consumed = self.decoder.frame_decode_batch(buf, L.FG_FRAME_CAPNP, final=False)
            n = len(offsets) - 1
            self.framer.end(buf, n, consumed, self.decoder.last_capnp_stop())
            data = np.frombuffer(buf[:consumed], np.uint8)
        else:
            data, offsets = self.framer.feed(chunk)
            n = len(offsets) - 1
            tab = self.decoder.decode_packed(data, offsets) if n else None
        if n == 0:
            return []
        blob, offs = tab.serialize(L.FG_CAPNP, data, offsets)
        raw = blob.tobytes()
        return [parse_canonical(raw[int(offs[i]):int(offs[i + 1])]) for i in range(n)]


class MultiCapnpSplitter(_EndingSplitter):
    """MultiStreamSplitter for CAP'N PROTO connections (input.format = "capnp": flowgger instances relaying to a collector): parks the
    chunks of many connections and hands them to the GPU together -- one fg_frame_decode_capnp_multi_batch call walks every
    connection's bytes as its own stream and decodes the messages.  Per connection the output is what a CapnpSplitter of its own
    returns for the bytes pushed so far: a Record (or the DecodeError the reference prints) per whole message; the bytes behind the
    last whole message are carried over to the connection's next chunk.  A table that ends the connection (512 or more segments, more
    than 8 Mi words) puts its CapnpStreamError last, behind the whole messages in front of it: later pushes raise ValueError.
    close(conn) ends the connection: its whole messages come with the next flush, carried bytes are dropped and nothing more is
    reported."""

    def __init__(self, decoder: Optional[CapnpDecoder] = None, policy: Optional[FlushPolicy] = None):
        super().__init__(decoder or CapnpDecoder(), policy)  # (_over: closed, or a table read_message refuses)

    def flush(self) -> list:
        """-> [(conn_id, [Record | DecodeError | CapnpStreamError, ...]), ...] for every connection that had chunks parked or was
        closed, in arrival order"""
        # a segment starts on a word of the buffer: the last len % 8 bytes can never complete a message and stay on the host
        conns, whole, raw, starts = self._take(align=8)
        if not conns:
            return []
        tab, offsets, kind, first, cons, stop = self.decoder.frame_decode_capnp_multi(raw, starts)
        can, coffs = b"", None
        if tab is not None:
            blob, coffs = tab.serialize(L.FG_CAPNP, np.frombuffer(raw + b"\0" * 32, np.uint8), offsets)
            can = blob.tobytes()
        out = []
        for k, c in enumerate(conns):
            res: list = [parse_canonical(can[int(coffs[i]):int(coffs[i + 1])]) for i in range(int(first[k]), int(first[k + 1]))
                         if kind[i] == L.FG_SLOT_FRAME]
            tail = whole[k][int(cons[k]):]
            over = c in self._closed
            if stop[k] in (L.FG_CAPNP_TOO_MANY_SEGMENTS, L.FG_CAPNP_TOO_LARGE):
                try:
                    CapnpFramer.frame(tail)  # (the text of the error: the few words of the table at `consumed`)
                    raise AssertionError("the framer stopped at a table the host walk accepts")
                except CapnpStreamError as e:
                    res.append(e)
                over = True
            self._closed.discard(c)
            if over:
                self._over.add(c)
            elif tail:
                self._carry[c] = tail
            out.append((c, res))
        return out


class CapnpTranscodingSplitter:
    """CapnpSplitter::run (splitter/capnp_splitter.rs:15-63) WITH the encoder: chunks of the stream in, the re-encoded + framed
    messages out.  handle_message + encoder.encode + the merger for every whole message of a chunk is one fg_transcode_batch
    (FG_CAPNP, FG_FRAME_NONE); the tables never leave the device.  ``feed`` returns a :class:`~flowgger_amd.encoder.Transcoded`
    (``.out`` the bytes for the output, ``.dec_status`` / ``.enc_status`` what the reference prints per dropped message)."""

    def __init__(self, encoder, decoder: Optional[CapnpDecoder] = None, device: int = 0, now_ts: float = 0.0, gpu_framing: bool = False):
        """gpu_framing: as for CapnpSplitter -- one fg_transcode_batch (FG_CAPNP, FG_FRAME_CAPNP) frames, decodes and encodes the chunk"""
        from .encoder import Pipeline

        self.decoder = decoder or CapnpDecoder(device=device)
        self.pipeline = Pipeline(self.decoder, encoder)
        self.framer = _GpuCapnpCarry() if gpu_framing else CapnpFramer()
        self.gpu_framing = gpu_framing
        self.now_ts = now_ts

    def feed(self, chunk: bytes):
        from .encoder import Transcoded

        if self.gpu_framing:
            buf = self.framer.begin(chunk)
            res = self.pipeline.run_stream(buf, L.FG_FRAME_CAPNP, final=False, now_ts=self.now_ts)
            self.framer.end(buf, len(res.out_offsets) - 1, res.consumed, self.decoder.last_capnp_stop())
            return res
        data, offsets = self.framer.feed(chunk)
        if len(offsets) < 2:  # no whole message yet
            return Transcoded(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint8), None, 0)
        return self.pipeline.run_packed(data, offsets, now_ts=self.now_ts)


class MultiTranscodingSplitter(_EndingSplitter):
    """MultiStreamSplitter / MultiSyslenSplitter / MultiCapnpSplitter WITH the encoder: parks the chunks of many connections and hands
    them to the GPU together -- one fg_transcode_multi_batch call frames every connection's bytes as its own stream, decodes the
    frames, encodes the Records and frames them for the output; the tables never leave the device.  flush() returns the bytes for the
    output -- what the connection threads of the reference would have sent for the bytes pushed so far, connection after connection in
    arrival order -- and per connection what they would have printed to stderr: DecodeError("<the decoder's or the encoder's error>:
    [<trimmed frame>]") per dropped frame (FG_FRAME_CAPNP: the error alone, capnp_splitter.rs:48-58), "Invalid UTF-8 input", and what
    ends a connection, as the decode-side classes state it: carry-over, close() and the end of a connection are theirs."""

    def __init__(self, decoder: Decoder, encoder, framing: int, policy: Optional[FlushPolicy] = None, now_ts: float = 0.0):
        from .encoder import Pipeline

        if framing not in (L.FG_FRAME_LINE, L.FG_FRAME_NUL, L.FG_FRAME_SYSLEN, L.FG_FRAME_CAPNP):
            raise ValueError("MultiTranscodingSplitter frames FG_FRAME_LINE, FG_FRAME_NUL, FG_FRAME_SYSLEN or FG_FRAME_CAPNP streams")
        if (framing == L.FG_FRAME_CAPNP) != (decoder.fmt == L.FG_CAPNP):
            raise ValueError("FG_FRAME_CAPNP streams are what a CapnpDecoder reads, and nothing else is")
        super().__init__(decoder, policy)
        self.pipeline, self.framing, self.now_ts = Pipeline(decoder, encoder), framing, now_ts
        self._extra = b""

    def _empty_message(self) -> list:
        """an empty octet-counted message in front of an EOF goes through the pipeline like any other: its bytes to the output, or
        its error"""
        t = self.pipeline.run_packed(np.zeros(16, np.uint8), np.zeros(2, np.uint64), now_ts=self.now_ts)
        if t.enc_status[0] == 0:
            self._extra = t.out.tobytes()
            return []
        return [self._decode_error(self._error(t, 0), b"")]

    def _error(self, t, i: int) -> str:
        from .encoder import Encoder

        st = int(t.dec_status[i])
        return self.decoder.error_string(st) if st else Encoder.error_string(int(t.enc_status[i]))

    def flush(self):
        """-> (bytes for the output, [(conn_id, [DecodeError | CapnpStreamError, ...]), ...] for every connection that had chunks parked
        or was closed, in arrival order)"""
        lines, syslen, capnp = self.framing in (L.FG_FRAME_LINE, L.FG_FRAME_NUL), self.framing == L.FG_FRAME_SYSLEN, self.framing == L.FG_FRAME_CAPNP
        # (a Cap'n Proto segment starts on a word of the buffer: the last len % 8 bytes can never complete a message and stay here)
        conns, segs, raw, starts = self._take(align=8 if capnp else 1)
        if not conns:
            return b"", []
        final = [1 if c in self._closed else 0 for c in conns] if lines else None  # (close(conn): its unterminated tail is a frame)
        t = self.pipeline.run_multi(raw, starts, final, self.framing, now_ts=self.now_ts)
        so, pieces, out = t.slot_offsets, [], []
        for k, c in enumerate(conns):
            a, b = int(t.seg_first[k]), int(t.seg_first[k + 1])
            pieces.append(t.out[int(t.out_offsets[a]):int(t.out_offsets[b])].tobytes())
            res: list = []
            over = False
            for i in range(a, b):
                kind = t.slot_kind[i]
                if kind == L.FG_SLOT_CARRY:
                    if lines:
                        self._carry[c] = raw[int(so[i]):int(so[i + 1])]
                elif kind == L.FG_SLOT_BAD_UTF8 and syslen:  # the reference's unwrap(): this connection's thread ends here
                    res.append(DecodeError(SYSLEN_PANIC))
                    over = True
                    break
                elif kind == L.FG_SLOT_BAD_UTF8:
                    res.append(DecodeError("Invalid UTF-8 input"))
                elif t.enc_status[i] != 0:
                    if capnp:
                        res.append(DecodeError(self._error(t, i)))
                        continue
                    if syslen:
                        sp = raw.index(b" ", int(so[i]))
                        frame = raw[sp + 1:sp + 1 + int(raw[int(so[i]):sp])]
                    else:
                        frame = self._unterminated(raw[int(so[i]):int(so[i + 1])], self.framing)
                    if self.framing == L.FG_FRAME_NUL and not self._trimmed(frame):
                        continue
                    res.append(self._decode_error(self._error(t, i), frame))
            if lines:  # (a closed connection is forgotten: MultiStreamSplitter)
                self._closed.discard(c)
                out.append((c, res))
                continue
            tail = segs[k][int(t.seg_consumed[k]):]
            if capnp:
                over = c in self._closed
                if t.seg_stop[k] in (L.FG_CAPNP_TOO_MANY_SEGMENTS, L.FG_CAPNP_TOO_LARGE):
                    try:
                        CapnpFramer.frame(tail)  # (the text of the error: the few words of the table at `consumed`)
                        raise AssertionError("the framer stopped at a table the host walk accepts")
                    except CapnpStreamError as e:
                        res.append(e)
                    over = True
            else:
                if not over and t.seg_stop[k] == L.FG_SYSLEN_BAD_LEN:
                    res.append(DecodeError(SYSLEN_BAD_LENGTH))
                    over = True
                if not over and c in self._closed:
                    res += self._eof(tail) if tail else [DecodeError(SYSLEN_BAD_LENGTH)]
                    pieces.append(self._extra)
                    self._extra = b""
                    over = True
            self._closed.discard(c)
            if over:
                self._over.add(c)
            elif tail:
                self._carry[c] = tail
            out.append((c, res))
        return b"".join(pieces), out


class RFC3164Decoder(Decoder):
    """src/flowgger/decoder/rfc3164_decoder.rs:10-213.  The reference's config is ignored (:13-15); two things it takes
    from its environment are explicit here: ``current_year`` (it reads the clock per parse, :179; default
    FG_YEAR_NOW: the library re-reads the UTC year at every decode call, so a long-lived decoder and its clones cross
    New Year like the reference; a fixed year is for tests / replays) and the IANA zone table behind ``time_tz::timezones::get_by_name`` (:195; default: every zone
    of the system tz database, flowgger_amd/tzdb.py).  {"rfc3164": {"current_year": 2020, "zones": [...] | None}}."""
    fmt = L.FG_RFC3164

    def __init__(self, config: Optional[dict] = None, device: int = 0):
        super().__init__(config, device)
        from . import tzdb

        opt = (config or {}).get("rfc3164", {})
        self.current_year = int(opt.get("current_year", L.FG_YEAR_NOW))
        zones = opt.get("zones", "all")
        self.tz_table = tzdb.default_table() if zones == "all" else (tzdb.build_table(zones) if zones else None)
        self._apply()

    def _apply(self):
        cfg = L.fg_rfc3164_cfg(self.current_year, None)
        t = self.tz_table
        if t is not None and len(t.names):
            names = (C.c_char_p * len(t.names))(*[n.encode() for n in t.names])
            zf = np.ascontiguousarray(t.zone_first, np.uint32)
            us = np.ascontiguousarray(t.utc_start, np.int64)
            uo = np.ascontiguousarray(t.utc_offset, np.int32)
            tab = L.fg_tz_table(len(t.names), C.cast(names, C.POINTER(C.c_char_p)), zf.ctypes.data, us.ctypes.data, uo.ctypes.data)
            cfg.tz = C.pointer(tab)
            self._keep3164 = (names, zf, us, uo, tab)
        L.check(L.lib().fg_set_rfc3164(self._ctx, C.byref(cfg)), "fg_set_rfc3164")

    def clone_boxed(self) -> "Decoder":
        other = super().clone_boxed()
        other.current_year, other.tz_table = self.current_year, self.tz_table
        return other


class LTSVDecoder(Decoder):
    """src/flowgger/decoder/ltsv_decoder.rs:17-221.  `config` mirrors the TOML tables
    ``input.ltsv_schema`` (name -> "string|bool|f64|i64|u64", case-insensitive, :33-45) and
    ``input.ltsv_suffixes`` (type -> suffix, :57-81): {"input": {"ltsv_schema": {...},
    "ltsv_suffixes": {...}}}."""
    fmt = L.FG_LTSV

    def _make_cfg(self, config: Optional[dict]):
        inp = (config or {}).get("input", {})
        schema = inp.get("ltsv_schema")
        suffixes = inp.get("ltsv_suffixes")
        cfg = L.fg_cfg()
        keep = []
        names, types = [], []
        if schema is not None:
            if not isinstance(schema, dict):
                raise ValueError("input.ltsv_schema must be a list of key/type pairs")
            for name, sdtype in schema.items():
                if not isinstance(sdtype, str):
                    raise ValueError("input.ltsv_schema types must be strings")
                t = _TYPE_IDS.get(sdtype.lower())
                if t is None:
                    raise ValueError(f"Unsupported type in input.ltsv_schema for name [{name}]")
                names.append(name.encode())
                types.append(t)
        cfg.n_schema = len(names)
        arr_n = (C.c_char_p * max(len(names), 1))(*names)
        arr_t = (C.c_uint8 * max(len(types), 1))(*types)
        cfg.schema_names = C.cast(arr_n, C.POINTER(C.c_char_p))
        cfg.schema_types = C.cast(arr_t, C.POINTER(C.c_uint8))
        keep += [arr_n, arr_t, names]
        if suffixes is not None:
            if not isinstance(suffixes, dict):
                raise ValueError("input.ltsv_suffixes must be a list of type/suffixes pairs")
            for sdtype, suffix in suffixes.items():
                if not isinstance(suffix, str):
                    raise ValueError("input.ltsv_suffixes suffixes must be strings")
                t = sdtype.lower()
                if t == "string":
                    raise ValueError("Strings cannot be suffixed")
                if t not in ("bool", "f64", "i64", "u64"):
                    raise ValueError(f"Unsupported type in input.ltsv_suffixes for type [{sdtype}]")
                setattr(cfg, "suffix_" + t, suffix.encode())
        self._keep = keep
        return cfg
