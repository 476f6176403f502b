"""The state blob of tfrec_amd_save_streams / tfrec_amd_load_streams (include/tfrec_amd.h): the 128-byte header
restated, and its parser.  The payload behind the header is opaque: only the library that wrote it reads it."""
from __future__ import annotations

import numpy as np

MAGIC = 0x54534654  # "TFST"
FORMAT = 1
HEADER_BYTES = 128

# tfrec_amd_state_header, little endian, packed as declared
HEADER_DTYPE = np.dtype([
    ("magic", "<u4"), ("format", "<u4"), ("version_hash", "<u8"),
    # the signature
    ("input_kind", "<i4"), ("format_in", "<i4"), ("format_pre", "<i4"), ("rate_p", "<i4"), ("rate_q", "<i4"),
    ("tail_bytes", "<i4"), ("pre_bytes", "<i4"), ("types_mask", "<u4"), ("flags", "<u4"), ("recorder", "<u4"),
    ("dc_windows", "<i4"), ("iq_windows", "<i4"), ("chain_state_bytes", "<u4"),
    ("payload_bytes", "<u4"), ("samples_since_restart", "<i8"),
    ("config", [("types_mask", "<i4"), ("thresh", "<i4"), ("filter_type", "<i4"), ("reserved", "<i4")]),
    ("tune_hz", "<i4"), ("tune_wide_hz", "<i4"), ("tune_input_hz", "<i4"), ("reserved", "u1", (20,)),
])
assert HEADER_DTYPE.itemsize == HEADER_BYTES
SIGNATURE_FIELDS = ("input_kind", "format_in", "format_pre", "rate_p", "rate_q", "tail_bytes", "pre_bytes", "types_mask", "flags",
                    "recorder", "dc_windows", "iq_windows", "chain_state_bytes")
INPUT_KINDS = ("u8", "10x", "resample", "format", "decimated")


def version_hash(version: bytes) -> int:
    """FNV-1a (64 bit) of the bytes of tfrec_amd_version()."""
    h = 0xCBF29CE484222325
    for b in bytes(version):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def parse_header(blob) -> dict:
    """One blob (bytes or a uint8 array, at least the header) -> its header's fields; `signature` is the tuple of the fields that
    must be equal in the source and the target context.  ValueError for a short blob, another magic or format, or a payload size
    that is not the blob's."""
    a = np.frombuffer(bytes(blob), dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
    if len(a) < HEADER_BYTES:
        raise ValueError("a state blob holds at least the %d-byte header, not %d bytes" % (HEADER_BYTES, len(a)))
    h = a[:HEADER_BYTES].view(HEADER_DTYPE)[0]
    if int(h["magic"]) != MAGIC:
        raise ValueError("magic 0x%08x, not 0x%08x" % (int(h["magic"]), MAGIC))
    if int(h["format"]) != FORMAT:
        raise ValueError("format %d, this parser reads %d" % (int(h["format"]), FORMAT))
    if int(h["payload_bytes"]) != len(a) - HEADER_BYTES:
        raise ValueError("payload_bytes %d, the blob has %d behind its header" % (int(h["payload_bytes"]), len(a) - HEADER_BYTES))
    out = {n: int(h[n]) for n in HEADER_DTYPE.names if n not in ("config", "reserved")}
    out["config"] = {n: int(h["config"][n]) for n in ("types_mask", "thresh", "filter_type", "reserved")}
    out["reserved"] = bytes(h["reserved"])
    out["signature"] = tuple(out[n] for n in SIGNATURE_FIELDS)
    return out
