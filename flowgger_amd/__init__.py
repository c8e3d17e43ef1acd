"""flowgger_amd -- MI355X (gfx950) bulk log-line decoder behind flowgger's Decoder/Record interface.

Scope: the per-line ``Decoder::decode()`` hot path (RFC5424, LTSV, GELF) of awslabs/flowgger,
rebuilt as hand-written HIP kernels behind a C ABI (include/fg_hip.h).  See DESIGN.md.
"""
from .record import DecodeError, Record, SDValue, StructuredData  # noqa: F401
from .decoder import (CapnpDecoder, CapnpFramer, CapnpSplitter, CapnpStreamError, CapnpTranscodingSplitter, Decoder, FlushPolicy, GelfDecoder,  # noqa: F401
                      LTSVDecoder, MultiCapnpSplitter, MultiStreamSplitter, MultiSyslenSplitter, MultiTranscodingSplitter, RFC3164Decoder, RFC5424Decoder, UdpUnpacker, pack_lines, pack_messages)
from .encoder import (CapnpEncoder, Encoder, GelfEncoder, LTSVEncoder, PassthroughEncoder, Pipeline,  # noqa: F401
                      RFC3164Encoder, RFC5424Encoder, Transcoded, TranscodedMulti, TranscodedUdp)

__all__ = ["Decoder", "RFC5424Decoder", "RFC3164Decoder", "LTSVDecoder", "GelfDecoder", "CapnpDecoder", "CapnpFramer", "CapnpSplitter",
           "CapnpStreamError", "CapnpTranscodingSplitter", "FlushPolicy", "MultiCapnpSplitter", "MultiStreamSplitter", "MultiSyslenSplitter", "MultiTranscodingSplitter", "UdpUnpacker", "pack_messages", "Record", "StructuredData",
           "SDValue", "DecodeError", "pack_lines", "Encoder", "GelfEncoder", "LTSVEncoder", "RFC5424Encoder",
           "RFC3164Encoder", "PassthroughEncoder", "CapnpEncoder", "Pipeline", "Transcoded", "TranscodedMulti", "TranscodedUdp"]
