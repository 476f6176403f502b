"""CPU restatement of the sample formats (include/tfrec_amd.h: tfrec_amd_create_format), in numpy.

A format maps one stored component (I or Q, little-endian, interleaved I, Q) to x, the int16 value every stage is defined on,
-8192 <= x <= 8191.  Written from the definition alone: nothing here calls the C library.

    u8   2 bytes per complex sample   x = (u8 - 128) << 6
    s8   2                            x = s8 << 6            (the u8 value of byte ^ 0x80)
    s16  4                            x = s16 >> 2, arithmetic shift
    f32  8                            v = f * 8192 in fp32; x = clamp(rint(v), -8192, 8191), ties to even; NaN -> 0

resample.resample_x16(to_x(fmt, raw), p, q) is then stage 0 of a rate context, to_x(fmt, raw) itself stage 0 at the base rate.
"""
from __future__ import annotations

import numpy as np

U8, S8, S16, F32 = 0, 1, 2, 3
NAMES = {U8: "u8", S8: "s8", S16: "s16", F32: "f32"}
FORMATS = {"u8": U8, "s8": S8, "s16": S16, "f32": F32, "cu8": U8, "cs8": S8, "cs16": S16, "cf32": F32}
_DTYPE = {U8: np.dtype("u1"), S8: np.dtype("i1"), S16: np.dtype("<i2"), F32: np.dtype("<f4")}


def _fmt(fmt) -> int:
    f = FORMATS[fmt] if isinstance(fmt, str) else int(fmt)
    if f not in NAMES:
        raise ValueError("unknown format %r" % (fmt,))
    return f


def bytes_per_sample(fmt) -> int:
    """Bytes of one complex sample."""
    return 2 * _DTYPE[_fmt(fmt)].itemsize


def components(fmt, raw_bytes) -> np.ndarray:
    """The stored components of a row of bytes, in the format's own type."""
    raw = np.ascontiguousarray(raw_bytes)
    return raw.reshape(-1).view(np.uint8).view(_DTYPE[_fmt(fmt)])


def to_x(fmt, raw_bytes) -> np.ndarray:
    """A row of bytes in the format -> x, interleaved int16 (I, Q)."""
    f = _fmt(fmt)
    c = components(f, raw_bytes)
    if f == U8:
        return ((c.astype(np.int32) - 128) << 6).astype(np.int16)
    if f == S8:
        return (c.astype(np.int32) << 6).astype(np.int16)
    if f == S16:
        return (c.astype(np.int32) >> 2).astype(np.int16)
    with np.errstate(over="ignore", invalid="ignore"):
        v = c.astype(np.float32) * np.float32(8192.0)  # fp32: exact, or +-inf
        r = np.clip(np.rint(v.astype(np.float64)), -8192.0, 8191.0)  # (rint of an fp32 value is the same in double)
    return np.where(np.isnan(v), 0.0, r).astype(np.int16)


def encode(fmt, x) -> np.ndarray:
    """The row of bytes (uint8) whose x is exactly the given int16 x (-8192 <= x <= 8191): x << 2 for s16, x / 8192 for f32,
    x >> 6 as int8 for s8 and (x >> 6) + 128 for u8, where x must be a multiple of 64."""
    f = _fmt(fmt)
    x = np.ascontiguousarray(x, dtype=np.int16).reshape(-1).astype(np.int32)
    assert x.min() >= -8192 and x.max() <= 8191
    if f in (U8, S8):
        assert not (x & 63).any(), "an 8-bit format holds multiples of 64"
        c = ((x >> 6) + (128 if f == U8 else 0)).astype(_DTYPE[f])
    elif f == S16:
        c = (x << 2).astype(_DTYPE[f])
    else:
        c = (x.astype(np.float32) / np.float32(8192.0)).astype(_DTYPE[f])  # exact: a 14-bit integer times 2^-13
    return c.view(np.uint8)
