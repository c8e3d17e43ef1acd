"""Host-side mirror of flowgger's Encoder / Merger interface for the GPU encode path.

Reference: ``trait Encoder { fn encode(&self, record: Record) -> Result<Vec<u8>, &'static str> }``
(src/flowgger/encoder/mod.rs:54-56) with GelfEncoder / LTSVEncoder / RFC5424Encoder / RFC3164Encoder /
PassthroughEncoder / CapnpEncoder, and ``trait Merger { fn frame(&self, bytes: &mut Vec<u8>) }`` (merger/mod.rs:30-32) with
LineMerger / NulMerger / SyslenMerger.  Here one call encodes AND frames a whole decoded batch on the GPU straight
from the decode tables (fg_encode_device): the result is one contiguous byte stream in input order, which is what
the outputs write.  Configuration keys are the reference's (output.gelf_extra, output.ltsv_extra, output.capnp_extra,
output.syslog_prepend_timestamp -- the latter as the already formatted header, since it is the wall clock).
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from . import _lib as L
from .tables import DeviceTables

# output.framing (merger/mod.rs:447-456): "noop" / "nop" / "capnp" are NopMerger, i.e. no framing
MERGERS = {None: L.FG_MERGE_NONE, "none": L.FG_MERGE_NONE, "noop": L.FG_MERGE_NONE, "nop": L.FG_MERGE_NONE, "capnp": L.FG_MERGE_NONE,
           "line": L.FG_MERGE_LINE, "nul": L.FG_MERGE_NUL, "syslen": L.FG_MERGE_SYSLEN}


def _compression(name: Optional[str]) -> int:
    """output.kafka_compression (kafka_output.rs:163-182: lowercased; "none" / "gzip" / "snappy", anything else panics)"""
    v = "none" if name is None else str(name).lower()
    if v == "none":
        return L.FG_COMP_NONE
    if v == "gzip":
        return L.FG_COMP_GZIP
    if v == "snappy":
        raise NotImplementedError("output.kafka_compression = \"snappy\" is not built")
    raise ValueError("Unsupported compression method")


def _wire(name: Optional[str]) -> int:
    """what the transcode calls hand out (fg_set_output_wire): "raw", the default, or "kafka" -- v0 message sets (see Pipeline)"""
    if name is None or name == "raw":
        return L.FG_WIRE_RAW
    if name == "kafka":
        return L.FG_WIRE_KAFKA_V0
    raise ValueError("wire must be \"raw\" or \"kafka\"")


def kafka_parse(buf: bytes):
    """a Kafka v0 message set -> [(crc_ok, attributes, value)] (null keys; for callers and tests, not for speed).  The offset field is
    not judged: a v0 producer may send anything there, the broker assigns it."""
    import struct
    import zlib

    out, at, over = [], 0, int(L.lib().fg_kafka_message_overhead())
    while at < len(buf):
        if len(buf) - at < over:
            raise ValueError("a message set ends inside a header")
        size, crc = struct.unpack_from(">iI", buf, at + 8)
        magic, attributes, keylen, vlen = struct.unpack_from(">bbii", buf, at + 16)
        end = at + over + vlen
        if magic != 0 or keylen != -1 or vlen < 0 or size != 14 + vlen or end > len(buf):
            raise ValueError(f"not a v0 message with a null key at byte {at}")
        out.append((zlib.crc32(buf[at + 16:end]) == crc, attributes, buf[at + over:end]))
        at = end
    return out


def _huffman(name: str) -> int:
    """how the compressor codes a block (fg_set_deflate_mode): "fixed", the default, or "dynamic" (see Pipeline)"""
    if name == "fixed":
        return L.FG_DEFLATE_FIXED
    if name == "dynamic":
        return L.FG_DEFLATE_DYNAMIC
    raise ValueError("huffman must be \"fixed\" or \"dynamic\"")


def _view(ptr, count, dt):
    """a copy of `count` elements of dtype `dt` at `ptr` (ctx-owned pinned memory a C call handed out); empty for none or NULL"""
    import numpy as np

    if not count or not ptr:
        return np.zeros(0, dt)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (count * np.dtype(dt).itemsize,)).view(dt).copy()


class Encoder:
    """Base class; subclasses fix ``enc`` (fg_encoder)."""
    enc = -1
    extra_key = None  # the output.* table with extra pairs, if the encoder has one

    def __init__(self, config: Optional[dict] = None, merger: Optional[str] = None, prepend: Optional[str] = None):
        out = (config or {}).get("output", {})
        extra = out.get(self.extra_key) if self.extra_key else None
        # the reference iterates a toml Table = BTreeMap: sorted by key
        self.extra = sorted((extra or {}).items())
        for k, v in self.extra:
            if not isinstance(v, str):  # gelf_encoder.rs:27-29 / ltsv_encoder.rs:21-23 / capnp_encoder.rs:23-25
                raise TypeError(f"output.{self.extra_key} values must be strings")
        self.merger = MERGERS[merger if merger is not None else out.get("framing")]
        self.prepend = prepend

    def _cfg_struct(self, now_ts: float = 0.0):
        """fg_encode_cfg for this encoder (+ the ctypes arrays that must stay alive while it is used)."""
        ks = (C.c_char_p * max(len(self.extra), 1))(*[k.encode() for k, _ in self.extra])
        vs = (C.c_char_p * max(len(self.extra), 1))(*[v.encode() for _, v in self.extra])
        cfg = L.fg_encode_cfg(self.enc, self.merger, len(self.extra), C.cast(ks, C.POINTER(C.c_char_p)),
                              C.cast(vs, C.POINTER(C.c_char_p)), None if self.prepend is None else self.prepend.encode(), now_ts)
        return cfg, (ks, vs)

    def encode_device(self, decoder, d_bytes, d_offsets, n: int, tables: DeviceTables, now_ts: float = 0.0, stream=None,
                      want_status: bool = False, out=None):
        """Encode + frame the n decoded lines of `tables` (produced by `decoder` from d_bytes / d_offsets).
        Returns (d_out uint8, d_out_offsets int64[n+1][, d_status uint8[n]]): message i = d_out[off[i]:off[i+1]],
        empty when the line's decode or encode failed (status 1 / fg_encode_error_string).
        `out` = an optional preallocated uint8 device tensor: one call (count, scan, write) when it is large
        enough; otherwise a sizing call comes first."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        cfg, _keep = self._cfg_struct(now_ts)
        d_off = torch.empty(n + 1, dtype=torch.int64, device=d_bytes.device)
        d_st = torch.empty(max(n, 1), dtype=torch.uint8, device=d_bytes.device) if want_status else None
        total = C.c_uint64()
        args = (decoder._ctx, decoder.fmt, C.byref(cfg), d_bytes.data_ptr(), d_bytes.numel(), d_offsets.data_ptr(), n,
                C.byref(tables.struct))
        tail = (d_off.data_ptr(), d_st.data_ptr() if want_status else None, C.byref(total), C.c_void_p(stream.cuda_stream))
        rc = L.FG_ERR_ENT_OVERFLOW
        if out is not None:
            rc = L.lib().fg_encode_device(*args, out.data_ptr(), out.numel(), *tail)
            if rc not in (L.FG_OK, L.FG_ERR_ENT_OVERFLOW):
                L.check(rc, "fg_encode_device")
        if rc == L.FG_ERR_ENT_OVERFLOW:
            if out is None:
                L.check(L.lib().fg_encode_device(*args, None, 0, *tail), "fg_encode_device (size)")
            out = torch.empty(max(int(total.value), 1), dtype=torch.uint8, device=d_bytes.device)
            L.check(L.lib().fg_encode_device(*args, out.data_ptr(), out.numel(), *tail), "fg_encode_device")
        res = (out[:int(total.value)], d_off)
        return res + (d_st[:n],) if want_status else res

    def encode_device_async(self, decoder, d_bytes, d_offsets, n: int, tables: DeviceTables, out, now_ts: float = 0.0, stream=None,
                            ent_hint: int = 0xFFFFFFFFFFFFFFFF):
        """fg_encode_device_async: count, scan and write queued on `stream`, no host synchronisation.  Returns (d_out_offsets
        int64[n+1], d_status uint8[n]); d_out_offsets[n] (device) = the bytes the batch needs -- when that exceeds out.numel()
        nothing was written to `out`.  ent_hint: an upper bound of the entries in `tables` (0 = none)."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        cfg, _keep = self._cfg_struct(now_ts)
        d_off = torch.empty(n + 1, dtype=torch.int64, device=d_bytes.device)
        d_st = torch.empty(max(n, 1), dtype=torch.uint8, device=d_bytes.device)
        L.check(L.lib().fg_encode_device_async(decoder._ctx, decoder.fmt, C.byref(cfg), d_bytes.data_ptr(), d_bytes.numel(), d_offsets.data_ptr(),
                                               n, C.byref(tables.struct), out.data_ptr(), out.numel(), d_off.data_ptr(), d_st.data_ptr(),
                                               ent_hint, C.c_void_p(stream.cuda_stream)), "fg_encode_device_async")
        return d_off, d_st[:n]

    @staticmethod
    def deflate_device(decoder, d_bytes, d_cuts, stream=None, out=None, huffman="fixed"):
        """fg_deflate_device: the resident bytes of `d_bytes` (uint8), cut into members by `d_cuts` (int64 / uint64 [n_members + 1],
        ascending byte bounds), as gzip members back to back -- what follows fg_encode_device when output.kafka_compression = "gzip".
        Returns (d_z uint8, d_z_offsets int64[n_members + 1]); an empty member produces no byte.  `out` = an optional preallocated
        uint8 device tensor: one call when it is large enough; otherwise a sizing call comes first.  huffman = "fixed" or "dynamic":
        fg_set_deflate_mode for this call (dynamic: every block the cheapest of stored, fixed and dynamic Huffman).  (`decoder` lends its
        ctx, which keeps the mode: every call sets it.)"""
        import torch

        L.check(L.lib().fg_set_deflate_mode(decoder._ctx, _huffman(huffman)), "fg_set_deflate_mode")
        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        n = d_cuts.numel() - 1
        d_zoff = torch.empty(n + 1, dtype=torch.int64, device=d_bytes.device)
        total = C.c_uint64()
        args = (decoder._ctx, d_bytes.data_ptr() if d_bytes.numel() else None, d_bytes.numel(), d_cuts.data_ptr(), n)
        tail = (d_zoff.data_ptr(), C.byref(total), C.c_void_p(stream.cuda_stream))
        return Encoder._sized_call(L.lib().fg_deflate_device, "fg_deflate_device", args, tail, total, out, d_bytes.device), d_zoff

    @staticmethod
    def _sized_call(fn, what, args, tail, total, out, device):
        """the contract of the resident calls: `out` when it is large enough, else a sizing call and a buffer of exactly the total"""
        import torch

        rc = L.FG_ERR_ENT_OVERFLOW
        if out is not None:
            rc = fn(*args, out.data_ptr(), out.numel(), *tail)
            if rc not in (L.FG_OK, L.FG_ERR_ENT_OVERFLOW):
                L.check(rc, what)
        if rc == L.FG_ERR_ENT_OVERFLOW:
            if out is None:
                L.check(fn(*args, None, 0, *tail), what + " (size)")
            out = torch.empty(max(int(total.value), 1), dtype=torch.uint8, device=device)
            L.check(fn(*args, out.data_ptr(), out.numel(), *tail), what)
        return out[:int(total.value)]

    @staticmethod
    def kafka_messageset_device(decoder, d_bytes, d_offsets, d_skip=None, stream=None, out=None):
        """fg_kafka_messageset_device: the resident values d_bytes[d_offsets[i] : d_offsets[i + 1]] (what encode_device returned) as a Kafka
        v0 message set -- every value behind its 26-byte header with its CRC-32, null keys.  d_skip: None, or uint8[n], nonzero = the row
        is not in the set (encode_device's status).  Returns (d_set uint8, d_set_offsets int64[n + 1]: where each row's message lies,
        an empty range for a skipped row).  `out` as in deflate_device.  (`decoder` lends its ctx.)"""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_bytes.device)
        n = d_offsets.numel() - 1
        d_soff = torch.empty(n + 1, dtype=torch.int64, device=d_bytes.device)
        total = C.c_uint64()
        args = (decoder._ctx, d_bytes.data_ptr() if d_bytes.numel() else None, d_bytes.numel(), d_offsets.data_ptr(),
                None if d_skip is None else d_skip.data_ptr(), n)
        tail = (d_soff.data_ptr(), C.byref(total), C.c_void_p(stream.cuda_stream))
        return Encoder._sized_call(L.lib().fg_kafka_messageset_device, "fg_kafka_messageset_device", args, tail, total, out, d_bytes.device), d_soff

    @staticmethod
    def kafka_wrap_device(decoder, d_z, d_z_offsets, stream=None, out=None):
        """fg_kafka_wrap_device: the gzip members d_z[d_z_offsets[m] : d_z_offsets[m + 1]] (what deflate_device made of a message set)
        each inside its wrapper message (attributes = 1, a CRC-32 over the compressed bytes); an empty member produces no byte.  Returns
        (d_w uint8, d_w_offsets int64[n_members + 1])."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(d_z.device)
        nm = d_z_offsets.numel() - 1
        d_woff = torch.empty(nm + 1, dtype=torch.int64, device=d_z.device)
        total = C.c_uint64()
        args = (decoder._ctx, d_z.data_ptr() if d_z.numel() else None, d_z_offsets.data_ptr(), nm)
        tail = (d_woff.data_ptr(), C.byref(total), C.c_void_p(stream.cuda_stream))
        return Encoder._sized_call(L.lib().fg_kafka_wrap_device, "fg_kafka_wrap_device", args, tail, total, out, d_z.device), d_woff

    @staticmethod
    def error_string(status: int) -> Optional[str]:
        s = L.lib().fg_encode_error_string(status)
        return None if s is None else s.decode()


class GelfEncoder(Encoder):  # encoder/gelf_encoder.rs
    enc, extra_key = L.FG_ENC_GELF, "gelf_extra"


class LTSVEncoder(Encoder):  # encoder/ltsv_encoder.rs
    enc, extra_key = L.FG_ENC_LTSV, "ltsv_extra"


class RFC5424Encoder(Encoder):  # encoder/rfc5424_encoder.rs
    enc = L.FG_ENC_RFC5424


class RFC3164Encoder(Encoder):  # encoder/rfc3164_encoder.rs
    enc = L.FG_ENC_RFC3164


class PassthroughEncoder(Encoder):  # encoder/passthrough_encoder.rs
    enc = L.FG_ENC_PASSTHROUGH


class CapnpEncoder(Encoder):  # encoder/capnp_encoder.rs: one Cap'n Proto message (record.capnp) per line
    enc, extra_key = L.FG_ENC_CAPNP, "capnp_extra"


class Transcoded:
    """Result of Pipeline.run: the encoded + framed stream and one verdict per line (copies of ctx-owned pinned memory)."""

    def __init__(self, out, out_offsets, meta, enc_status, frame_offsets, consumed):
        self.out, self.out_offsets, self.meta, self.enc_status = out, out_offsets, meta, enc_status
        self.frame_offsets, self.consumed = frame_offsets, consumed

    @property
    def n(self) -> int:
        return len(self.enc_status)

    @property
    def dec_status(self):
        return (self.meta & 0xFF).astype("uint8")

    def message(self, i: int) -> bytes:
        return self.out[int(self.out_offsets[i]):int(self.out_offsets[i + 1])].tobytes()

    # With compression set on the Pipeline `out` is None and the stream comes as gzip members: z (uint8), z_offsets[n_members + 1],
    # member_first[n_members + 1] (each member's first message index; the last entry = n), raw_bytes (the uncompressed total).
    # With wire = "kafka" on the Pipeline (.wire says so) a member is Kafka v0 wire bytes: a plain message set without compression, one
    # gzip wrapper message around the inner set with it; rows with enc_status != 0 are in no set.
    z = z_offsets = member_first = None
    raw_bytes = 0
    wire = "raw"

    def members(self):
        """the members, one `bytes` each: gzip members (every one inflates on its own), or, with wire = "kafka", the wire bytes of each"""
        z = self.z.tobytes()
        return [z[int(self.z_offsets[k]):int(self.z_offsets[k + 1])] for k in range(len(self.z_offsets) - 1)]

    def kafka_records(self):
        """wire = "kafka": per member, the list of (crc_ok, value) of its inner messages -- the plain set parsed, or the wrapper parsed,
        its value inflated with Python's zlib and the inner set parsed (crc_ok then covers both CRCs).  For callers and tests."""
        import zlib

        if self.wire != "kafka":
            raise ValueError("not a wire = \"kafka\" result")
        out = []
        for m in self.members():
            msgs = kafka_parse(m)
            if len(msgs) == 1 and msgs[0][1] == 1:
                ok = msgs[0][0]
                out.append([(ok and iok, v) for iok, _, v in kafka_parse(zlib.decompress(msgs[0][2], 31))])
            else:
                out.append([(iok, v) for iok, _, v in msgs])
        return out

    def messages(self):
        """the messages of a compressed or wire result, inflated with Python's zlib (for callers and tests, not for speed): split by
        out_offsets, or, with wire = "kafka", the values of the sets' messages in row order, b"" for a row that is in no set"""
        import zlib

        if self.wire == "kafka":
            vals = iter(v for member in self.kafka_records() for _, v in member)
            return [b"" if self.enc_status[i] else next(vals) for i in range(self.n)]
        raw = b"".join(zlib.decompress(m, 31) for m in self.members() if m)
        return [raw[int(self.out_offsets[i]):int(self.out_offsets[i + 1])] for i in range(self.n)]


class TranscodedMulti(Transcoded):
    """Result of Pipeline.run_multi: Transcoded (one verdict per SLOT, no frame_offsets / consumed) plus the lists of the segmented
    framers -- slot_offsets (LINE / NUL / CAPNP: n + 1 slot bounds in the buffer; SYSLEN: n frame starts, prefix included), slot_kind
    (FG_SLOT_*), seg_first [K + 1], seg_consumed [K], seg_stop [K] (FG_SYSLEN_* / FG_CAPNP_*; None for LINE / NUL)."""

    def __init__(self, out, out_offsets, meta, enc_status, slot_offsets, slot_kind, seg_first, seg_consumed, seg_stop):
        super().__init__(out, out_offsets, meta, enc_status, None, None)
        self.slot_offsets, self.slot_kind = slot_offsets, slot_kind
        self.seg_first, self.seg_consumed, self.seg_stop = seg_first, seg_consumed, seg_stop


class TranscodedUdp(Transcoded):
    """Result of Pipeline.run_datagrams: Transcoded (one verdict per DATAGRAM, no frame_offsets) plus udp_status (FG_UDP_*: why a
    datagram was dropped before the decoder saw it)."""

    def __init__(self, out, out_offsets, meta, enc_status, consumed, udp_status, fmt):
        super().__init__(out, out_offsets, meta, enc_status, None, consumed)
        self.udp_status, self._fmt = udp_status, fmt

    def stderr_lines(self):
        """what the reference writes to stderr for the batch, in order: per datagram that produced nothing, the bare error
        (input/udp_input.rs:84-86 prints `{e}` alone) -- of the gate / inflater / UTF-8 check, else of the decoder, else of the encoder"""
        lib, out = L.lib(), []
        for i in range(self.n):
            if self.udp_status[i] > L.FG_UDP_GZIP:
                out.append(lib.fg_udp_error_string(int(self.udp_status[i])).decode())
            elif self.meta[i] & 0xFF:
                out.append(lib.fg_error_string(self._fmt, int(self.meta[i] & 0xFF)).decode())
            elif self.enc_status[i]:
                out.append(lib.fg_encode_error_string(int(self.enc_status[i])).decode())
        return out


class Pipeline:
    """decoder -> encoder -> merger for whole batches with HOST buffers (fg_transcode_batch): what
    ``handle_line`` (splitter/line_splitter.rs:44-54) does per line.  Only the encoded bytes and the per-line
    verdicts come back over PCIe; the decode tables stay in HBM."""

    def __init__(self, decoder, encoder: Encoder, compression: Optional[str] = None, coalesce: int = 1, member_bytes: int = 0,
                 huffman: str = "fixed", wire: str = "raw"):
        """compression: None / "none", or "gzip" -- the encoded stream is deflated on the GPU and comes back as gzip members instead of
        `.out` (fg_set_output_compression): one member per `coalesce` messages (the reference's output.kafka_coalesce), or, with
        coalesce = 0, members of about `member_bytes` bytes cut at message boundaries (0 = one block of the compressor).  huffman:
        "fixed" (the default) or "dynamic" -- dynamic Huffman blocks where they are smaller (fg_set_deflate_mode): fewer bytes, more
        compressor time.  wire: "raw" (the default) or "kafka" -- the messages come back as Kafka v0 message sets (fg_set_output_wire)
        instead of `.out`, one set per member of the policy above: plain, or with compression each deflated and inside its wrapper
        message, which is what a broker takes."""
        self.decoder, self.encoder = decoder, encoder
        self.wire = _wire(wire)
        self._merger = None  # from_config with the Kafka output: the FG_MERGE_* to encode with in place of the encoder's own
        self.huffman = _huffman(huffman)
        self.compression = _compression(compression)
        self.coalesce, self.member_bytes = int(coalesce), int(member_bytes)
        if self.coalesce < 0 or self.member_bytes < 0:
            raise ValueError("coalesce and member_bytes must not be negative")

    @classmethod
    def from_config(cls, decoder, encoder: Encoder, config: Optional[dict]):
        """output.kafka_compression ("none" / "gzip", any case; "snappy" is not built) and output.kafka_coalesce (default 1), as
        output/kafka_output.rs:163-182 reads them"""
        out = (config or {}).get("output", {})
        kw = dict(compression=str(out.get("kafka_compression", "none")), coalesce=int(out.get("kafka_coalesce", 1)))
        if out.get("type") == "kafka":
            # output.type = "kafka": v0 message sets, and the encoder's merger is left out of the values -- on the pipeline's own copy of
            # the cfg, the caller's Encoder stays as it is (kafka_output.rs:199-202 ignores output.framing and says so)
            import sys

            if encoder.merger != L.FG_MERGE_NONE:
                print("Output framing is ignored with the Kafka output", file=sys.stderr)
            kw.update(wire="kafka")
        p = cls(decoder, encoder, **kw)
        if p.wire == L.FG_WIRE_KAFKA_V0:
            p._merger = L.FG_MERGE_NONE
        return p

    def _encode_cfg(self, now_ts: float):
        cfg, keep = self.encoder._cfg_struct(now_ts)
        if self._merger is not None:
            cfg.merger = self._merger
        return cfg, keep

    def _set_compression(self):
        # (the setting lives on the decoder's ctx, which Pipelines may share: set for every call)
        cfg = L.fg_compress_cfg(self.compression, self.coalesce, self.member_bytes)
        L.check(L.lib().fg_set_output_compression(self.decoder._ctx, C.byref(cfg)), "fg_set_output_compression")
        L.check(L.lib().fg_set_deflate_mode(self.decoder._ctx, self.huffman), "fg_set_deflate_mode")
        L.check(L.lib().fg_set_output_wire(self.decoder._ctx, self.wire), "fg_set_output_wire")

    def _transcode(self, what: str, now_ts: float, call):
        """one transcode call: the encode cfg built, the ctx's output settings set, `call(ctx, fmt, cfg)` -- the C call itself, which the
        caller spells out -- made and its return code checked"""
        cfg, _keep = self._encode_cfg(now_ts)
        self._set_compression()
        L.check(call(self.decoder._ctx, self.decoder.fmt, C.byref(cfg)), what)

    def _compressed(self, t: Transcoded) -> Transcoded:
        """with compression set: the members of the call that produced `t` in place of its `out`"""
        import numpy as np

        if self.compression == L.FG_COMP_NONE and self.wire == L.FG_WIRE_RAW:
            return t
        t.wire = "kafka" if self.wire == L.FG_WIRE_KAFKA_V0 else "raw"
        c = L.fg_compressed()
        L.check(L.lib().fg_last_compressed(self.decoder._ctx, C.byref(c)), "fg_last_compressed")
        nm = int(c.n_members)
        t.out = None
        t.z = _view(c.z, int(c.z_bytes), np.uint8)
        t.z_offsets = _view(c.z_offsets, nm + 1, np.uint64) if nm else np.zeros(1, np.uint64)
        t.member_first = _view(c.member_first, nm + 1, np.uint64) if nm else np.zeros(1, np.uint64)
        t.raw_bytes = int(c.raw_bytes)
        return t

    def _call(self, framing: int, data, nbytes: int, offsets, n: int, final: bool, now_ts: float) -> Transcoded:
        import numpy as np

        res = L.fg_transcoded()
        self._transcode("fg_transcode_batch", now_ts, lambda ctx, fmt, cfg: L.lib().fg_transcode_batch(
            ctx, fmt, framing, cfg, data.ctypes.data, nbytes, None if offsets is None else offsets.ctypes.data, n, int(final), C.byref(res)))
        m = int(res.n)
        return self._compressed(Transcoded(_view(res.out, int(res.out_bytes), np.uint8),
                                           _view(res.out_offsets, m + 1 if m else 0, np.uint64) if m else np.zeros(1, np.uint64),
                                           _view(res.meta, m, np.uint32), _view(res.enc_status, m, np.uint8),
                                           _view(res.frame_offsets, m + 1, np.uint64) if (m and res.frame_offsets) else None, int(res.consumed)))

    def run_packed(self, data, offsets, now_ts: float = 0.0) -> Transcoded:
        """framed lines (packed bytes + offsets[n + 1], as produced by pack_lines)"""
        import numpy as np

        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        return self._call(L.FG_FRAME_NONE, data, int(offsets[-1]) if n else 0, offsets, n, True, now_ts)

    def run_stream(self, raw, framing: int, final: bool = True, now_ts: float = 0.0) -> Transcoded:
        """a raw stream chunk, framed on the GPU ("\\n" / NUL / FG_FRAME_SYSLEN: "<len> " prefixes -- `.frame_offsets` are then the frame
        starts, prefixes included, and decoder.last_syslen_stop() says how the chain ended; FG_FRAME_CAPNP with a CapnpDecoder: the segment
        tables of a Cap'n Proto stream -- `.frame_offsets` are the message starts and decoder.last_capnp_stop() says how the chain
        ended); bytes past `.consumed` belong to the next chunk"""
        import numpy as np

        data = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw, dtype=np.uint8)
        if len(data) == 0:
            data = np.zeros(1, np.uint8)
            return self._call(framing, data, 0, None, 0, final, now_ts)
        return self._call(framing, data, len(data), None, 0, final, now_ts)

    def run_multi(self, raw, seg_starts, seg_final, framing: int, now_ts: float = 0.0) -> TranscodedMulti:
        """fg_transcode_multi_batch: the chunks of K connections back to back (connection k = raw[seg_starts[k]:seg_starts[k + 1]]),
        every one framed as a stream of its own ("\\n" / NUL with seg_final[k] != 0: its unterminated tail is a frame; FG_FRAME_SYSLEN;
        FG_FRAME_CAPNP with a CapnpDecoder, starts on multiples of 8 -- seg_final must be None for both), decoded and encoded: `.out`
        is what the K connection threads of the reference would have sent, in buffer order.  An octet-counted connection ends at its
        first payload that is not UTF-8 (FG_SLOT_BAD_UTF8); its later frames are FG_SLOT_UNREACHED and produce nothing."""
        import numpy as np

        data = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw, dtype=np.uint8)
        starts = np.ascontiguousarray(seg_starts, dtype=np.uint64)
        K = len(starts) - 1
        final = None if seg_final is None else np.ascontiguousarray(seg_final, dtype=np.uint8)
        res = L.fg_transcoded_multi()
        self._transcode("fg_transcode_multi_batch", now_ts, lambda ctx, fmt, cfg: L.lib().fg_transcode_multi_batch(
            ctx, fmt, framing, cfg, data.ctypes.data if data.size else None, data.size, starts.ctypes.data,
            final.ctypes.data if final is not None and K else None, K, C.byref(res)))
        m = int(res.n)
        syslen = framing == L.FG_FRAME_SYSLEN
        return self._compressed(TranscodedMulti(_view(res.out, int(res.out_bytes), np.uint8), _view(res.out_offsets, m + 1, np.uint64),
                                                _view(res.meta, m, np.uint32), _view(res.enc_status, m, np.uint8),
                                                _view(res.slot_offsets, m if syslen else m + 1, np.uint64), _view(res.slot_kind, m, np.uint8),
                                                _view(res.seg_first, K + 1, np.uint64), _view(res.seg_consumed, K, np.uint64),
                                                _view(res.seg_stop, K, np.uint8) if res.seg_stop else None))

    def run_datagrams(self, datagrams, max_inflated=None, now_ts: float = 0.0) -> TranscodedUdp:
        """fg_udp_transcode_batch: the body of the UDP input's receive loop (input/udp_input.rs:66-143) for a batch -- a list of
        datagrams, or (data uint8, offsets uint64[n + 1]) with the datagrams back to back; each a zlib stream, a gzip member or a
        bare record.  `.out` is what the reference sends for them, `.stderr_lines()` what it prints.  max_inflated: the most a
        compressed datagram may inflate to (None = 65 527 * 5)."""
        import numpy as np

        from .decoder import pack_lines

        if isinstance(datagrams, tuple):
            data, offsets = datagrams
        else:
            data, offsets = pack_lines(list(datagrams))
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        nbytes = int(offsets[-1]) if n else 0
        res, ust = L.fg_transcoded(), C.c_void_p()
        self._transcode("fg_udp_transcode_batch", now_ts, lambda ctx, fmt, cfg: L.lib().fg_udp_transcode_batch(
            ctx, fmt, cfg, data.ctypes.data if nbytes else None, nbytes, offsets.ctypes.data, n, int(max_inflated or 0), C.byref(res), C.byref(ust)))
        return self._compressed(TranscodedUdp(_view(res.out, int(res.out_bytes), np.uint8),
                                              _view(res.out_offsets, n + 1, np.uint64) if n else np.zeros(1, np.uint64),
                                              _view(res.meta, n, np.uint32), _view(res.enc_status, n, np.uint8), int(res.consumed), _view(ust, n, np.uint8),
                                              self.decoder.fmt))
