"""The Kafka v0 message-set wire format from the protocol guide, in plain Python (struct and zlib.crc32): the independent reference the
message-set kernels are held against.  Nothing here calls the library.

A message, all integers big-endian:  offset 8 (0) | message_size 4 (14 + value length) | crc 4 | magic 1 (0) | attributes 1 | key length 4
(-1: a null key) | value length 4 | value.  crc = CRC-32 of magic .. the value's end.  A message set is messages back to back; a gzip
wrapper is one message with attributes = 1 whose value is a gzip member that holds a message set."""
from __future__ import annotations

import struct
import zlib

OVERHEAD = 26
ATTR_PLAIN, ATTR_GZIP = 0, 1


def message(value: bytes, attributes: int = ATTR_PLAIN) -> bytes:
    body = struct.pack(">bbii", 0, attributes, -1, len(value)) + value
    return struct.pack(">qiI", 0, 4 + len(body), zlib.crc32(body)) + body


def message_set(values, skip=None) -> bytes:
    """the set of the values whose skip flag is not set (skip: None or one flag per value)"""
    return b"".join(message(v) for i, v in enumerate(values) if not (skip is not None and skip[i]))


def set_offsets(values, skip=None):
    """where each row's message lies in message_set(values, skip): n + 1 bounds, an empty range for a skipped row"""
    out = [0]
    for i, v in enumerate(values):
        out.append(out[-1] + (0 if skip is not None and skip[i] else OVERHEAD + len(v)))
    return out


def wrapper(gzip_member: bytes) -> bytes:
    return message(gzip_member, ATTR_GZIP)


def parse_set(buf: bytes):
    """-> [(crc_ok, attributes, value)]; raises ValueError for anything that is not a whole v0 message set with null keys"""
    buf = bytes(buf)
    out, at = [], 0
    while at < len(buf):
        if len(buf) - at < OVERHEAD:
            raise ValueError(f"{len(buf) - at} bytes left at {at}: less than a header")
        offset, size, crc = struct.unpack_from(">qiI", buf, at)
        magic, attributes, keylen, vlen = struct.unpack_from(">bbii", buf, at + 16)
        if offset != 0 or magic != 0 or keylen != -1 or vlen < 0 or size != 14 + vlen or at + OVERHEAD + vlen > len(buf):
            raise ValueError(f"message at {at}: offset {offset} size {size} magic {magic} key length {keylen} value length {vlen}")
        end = at + OVERHEAD + vlen
        out.append((zlib.crc32(buf[at + 16:end]) == crc, attributes, buf[at + OVERHEAD:end]))
        at = end
    return out


def records(member: bytes):
    """what a consumer gets out of one member as the transcode calls hand it out: [(crc_ok, value)] of the inner messages.  The member is
    a plain message set, or ONE gzip wrapper whose value inflates (as a single gzip member, nothing left over) to one; crc_ok of a
    record inside a wrapper is its own CRC's and the wrapper's"""
    msgs = parse_set(member)
    if len(msgs) == 1 and msgs[0][1] == ATTR_GZIP:
        ok, _, z = msgs[0]
        d = zlib.decompressobj(31)
        inner = d.decompress(z)
        if not d.eof or d.unused_data:
            raise ValueError("the wrapper's value is not one whole gzip member")
        return [(ok and iok, v) for iok, attr, v in _plain(parse_set(inner))]
    return [(ok, v) for ok, attr, v in _plain(msgs)]


def _plain(msgs):
    for m in msgs:
        if m[1] != ATTR_PLAIN:
            raise ValueError(f"attributes {m[1]} inside a set")
    return msgs
