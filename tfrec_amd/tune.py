"""Digital tuning (tfrec_amd_tune_streams): the numpy restatement of the frequency shift the front end applies
to a tuned stream's 1.536 MS/s int16 (I, Q) input before the decimating FIR.

    inc   = floor((tune_hz * 2^33 + 1536000) / 3072000) mod 2^32
    p     = (n * inc) mod 2^32,  k = p >> 20            (n: complex sample since the stream's start or last restart)
    C[k]  = round(32767 * cos(2 pi k / 4096)),  S[k] = C[(k - 1024) mod 4096]
    I'    = sat16((I * C[k] + Q * S[k] + 2^14) >> 15)
    Q'    = sat16((Q * C[k] - I * S[k] + 2^14) >> 15)

A signal at +tune_hz in the recording ends up at DC; tune_hz = 0 leaves the stream untouched.

Wideband tune (tfrec_amd_tune_streams_wide): the same mixer at the 15.36 MS/s input rate, ahead of the 10:1 stage
of TFREC_AMD_F_INPUT_10X -- inc10, mix10_s16 -- and that stage itself on int16 input, decim10_s16:

    inc10 = floor((tune_hz * 2^33 + 15360000) / 30720000) mod 2^32
    y0[m] = int16( sum_{n<60} ( x'[10 m - 50 + n] * h10[n] ) >> 16 )       (x' = 0 before the stream's start)

Input-rate tune (tfrec_amd_tune_streams_input): the same mixer at the input rate 1536000 P / Q of a rate context,
ahead of the resampling stage -- inc_in, mix_in_s16; the stage on int16 input is resample.resample_x16:

    inc_in = floor((tune_hz * 2^33 * Q + 1536000 P) / (2 * 1536000 P)) mod 2^32,    2 |tune_hz| Q < 1536000 P"""
from __future__ import annotations

import numpy as np

RATE = 1536000  # complex samples per second entering downconvert::process_iq
TABLE_BITS = 12
TUNE_MAX = RATE // 2  # |tune_hz| < TUNE_MAX


def table():
    """(C, S) as int32 arrays of 4096 entries: C[k] = round(32767 cos(2 pi k / 4096)), S[k] = C[(k - 1024) mod 4096]."""
    k = np.arange(1 << TABLE_BITS)
    c = np.round(32767.0 * np.cos(2.0 * np.pi * k / (1 << TABLE_BITS))).astype(np.int32)
    s = c[(k - (1 << (TABLE_BITS - 2))) % (1 << TABLE_BITS)]
    return c, s


def inc(tune_hz: int) -> int:
    """The phase increment per complex sample, in units of 2^-32 turns (exact integers, floor division)."""
    t = int(tune_hz)
    if not -TUNE_MAX < t < TUNE_MAX:
        raise ValueError("tune_hz %d outside (-%d, %d)" % (t, TUNE_MAX, TUNE_MAX))
    return ((t << 33) + RATE) // (2 * RATE) % (1 << 32)


def _mix(x16, step: int, n0: int) -> np.ndarray:
    x = np.ascontiguousarray(x16, dtype=np.int16).reshape(-1)
    assert x.size % 2 == 0
    if step == 0:
        return x.copy()
    n = (np.arange(x.size // 2, dtype=np.uint64) + np.uint64(int(n0) % (1 << 32))) & np.uint64(0xFFFFFFFF)
    p = (n * np.uint64(step)) & np.uint64(0xFFFFFFFF)
    k = (p >> np.uint64(32 - TABLE_BITS)).astype(np.int64)
    c, s = table()
    ck, sk = c[k].astype(np.int64), s[k].astype(np.int64)
    i, q = x[0::2].astype(np.int64), x[1::2].astype(np.int64)
    out = np.empty_like(x)
    out[0::2] = np.clip((i * ck + q * sk + (1 << 14)) >> 15, -32768, 32767)
    out[1::2] = np.clip((q * ck - i * sk + (1 << 14)) >> 15, -32768, 32767)
    return out


def mix_s16(x16, tune_hz: int, n0: int = 0) -> np.ndarray:
    """Interleaved int16 (I, Q) samples x16, the first of them sample n0 of its stream -> the tuned samples (int16, same
    layout).  tune_hz = 0: a copy of x16."""
    return _mix(x16, inc(tune_hz), n0)


RATE10 = 10 * RATE  # complex samples per second of the TFREC_AMD_F_INPUT_10X input
TUNE10_MAX = RATE10 // 2  # |tune_hz| < TUNE10_MAX for the wide tune


def inc10(tune_hz: int) -> int:
    """The wide tune's phase increment per 15.36 MS/s sample, in units of 2^-32 turns."""
    t = int(tune_hz)
    if not -TUNE10_MAX < t < TUNE10_MAX:
        raise ValueError("tune_hz %d outside (-%d, %d)" % (t, TUNE10_MAX, TUNE10_MAX))
    return ((t << 33) + RATE10) // (2 * RATE10) % (1 << 32)


def mix10_s16(x16, tune_hz: int, n0: int = 0) -> np.ndarray:
    """mix_s16 at the input rate: x16 are 15.36 MS/s samples, the first of them INPUT sample n0 of its stream."""
    return _mix(x16, inc10(tune_hz), n0)


def inc_in(tune_hz: int, p: int, q: int) -> int:
    """The input-rate tune's phase increment per sample at 1536000 p / q samples per second, in units of 2^-32 turns."""
    t, p, q = int(tune_hz), int(p), int(q)
    if p <= 0 or q <= 0:
        raise ValueError("rate %d/%d" % (p, q))
    if not 2 * abs(t) * q < RATE * p:
        raise ValueError("tune_hz %d outside half the input rate %d * %d / %d" % (t, RATE, p, q))
    return ((t << 33) * q + RATE * p) // (2 * RATE * p) % (1 << 32)


def mix_in_s16(x16, tune_hz: int, p: int, q: int, n0: int = 0) -> np.ndarray:
    """mix_s16 at the input rate 1536000 p / q: x16 are samples at that rate, the first of them INPUT sample n0 of its stream."""
    return _mix(x16, inc_in(tune_hz, p, q), n0)


def taps10() -> np.ndarray:
    """The 60 taps of the 10:1 stage, read from the kernel's source (csrc/frontend.hip: kTaps10)."""
    import os
    import re

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "frontend.hip")) as f:
        m = re.search(r"kTaps10\[60\]\s*=\s*\{([^}]*)\}", f.read())
    h = np.array([int(v) for v in m.group(1).replace("\n", " ").split(",") if v.strip()], dtype=np.int64)
    assert h.size == 60
    return h


def decim10_s16(x16, hist=None) -> np.ndarray:
    """The 10:1 stage on interleaved int16 (I, Q) input at 15.36 MS/s: y0[m] = int16(sum_n (x[10 m - 50 + n] * h10[n]) >> 16),
    per-tap arithmetic shift, int16 store.  hist: the 50 complex samples (100 int16) before x16, default silence (a stream's
    start).  The number of complex input samples must be a multiple of 10."""
    x = np.ascontiguousarray(x16, dtype=np.int16).reshape(-1, 2).astype(np.int64)
    assert x.shape[0] % 10 == 0
    h0 = np.zeros((50, 2), dtype=np.int64) if hist is None else np.asarray(hist, dtype=np.int64).reshape(50, 2)
    xx = np.concatenate([h0, x])
    m = x.shape[0] // 10
    acc = np.zeros((m, 2), dtype=np.int64)
    for n, hn in enumerate(taps10()):
        acc += (xx[n: n + 10 * m: 10] * hn) >> 16
    return acc.astype(np.int16).reshape(-1)


def s16_of_u8(iq) -> np.ndarray:
    """The default input as the front end sees it: x = (u8 - 128) << 6 (engine.cpp:77-78), interleaved int16."""
    return ((np.asarray(iq, dtype=np.int16) - 128) << 6).astype(np.int16)
