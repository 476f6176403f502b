"""CPU restatement of the resampling stage (include/tfrec_amd.h: tfrec_amd_create_rate), in numpy integers.

A context created for the input rate fs_in = 1536000 * P / Q takes u8 IQ at that rate and resamples it to the 1.536 MS/s
int16 stream that enters downconvert::process_iq.  The stage has no reference counterpart: it is defined here, in the
reference's FIR style (int taps, arithmetic >> 16 per tap, int16 store), and the GPU kernel is pinned to this file bit for bit.
Written from the definition alone: nothing here calls the C library.

    r = P / Q (input samples per output sample), gcd(P, Q) = 1, 1 < r < 10, and Q <= 64 or Q divides 1536 -- the latter is
        "fs_in is a whole number of kHz": 2.0, 2.5, 5, 10, 12.5 MS/s are 125/96, 625/384, 625/192, 625/96, 3125/384
    T = 2 * ceil(3 r) taps per phase
    output m (since the stream's start or last restart):  a = m P,  i0 = a div Q,  phi = a mod Q
    y0[m] = int16( sum_{n<T} ( x[i0 - (T-1) + n] * h[phi][n] ) >> 16 )   per rail, x = (u8 - 128) << 6, x[<0] = 0
    on int16 input x' (the input-rate tune of DESIGN.md 6g ahead of the stage): the same sum over x' -- resample_x16
    h[phi][n]: d = n - T/2 + 1 - phi/Q, g = sinc(d / r) (0.54 + 0.46 cos(2 pi d / T)), v = g 65536 / sum_n g, h = round(v),
               the residual 65536 - sum_n h added to the tap with the largest v (the lowest n among equals)
"""
from __future__ import annotations

import math

import numpy as np

BASE_RATE = 1536000
Q_MAX = 64  # every denominator up to here ...
Q_DIV = 1536  # ... and every divisor of this one
TIE_EPS = 1e-9


class RateError(ValueError):
    """A rate outside the definition, or one the definition refuses."""


def reduce_rate(rate_hz: int) -> tuple[int, int]:
    """A sample rate in Hz -> (P, Q) in lowest terms, rate = 1536000 P / Q."""
    g = math.gcd(int(rate_hz), BASE_RATE)
    return int(rate_hz) // g, BASE_RATE // g


def n_taps(p: int, q: int) -> int:
    """T, the taps per phase; raises RateError for a rate outside the supported range."""
    p, q = int(p), int(q)
    if p <= 0 or q <= 0 or (q > Q_MAX and Q_DIV % q) or math.gcd(p, q) != 1 or not (q < p < 10 * q):
        raise RateError("unsupported rate %d/%d" % (p, q))
    return 2 * ((3 * p + q - 1) // q)


def taps(p: int, q: int) -> np.ndarray:
    """h[phi][n] as int32 [Q, T]; raises RateError for a refused rate."""
    t = n_taps(p, q)
    h = np.empty((q, t), dtype=np.int32)
    for phi in range(q):
        g = []
        for n in range(t):
            dn = (n - t // 2 + 1) * q - phi  # d = dn / Q, d / r = dn / P
            s = 1.0 if dn == 0 else math.sin(math.pi * dn / p) / (math.pi * dn / p)
            g.append(s * (0.54 + 0.46 * math.cos(2.0 * math.pi * dn / (q * t))))
        total = math.fsum(g)
        v = [x * 65536.0 / total for x in g]
        for x in v:
            if abs(abs(x - math.floor(x)) - 0.5) < TIE_EPS:
                raise RateError("rate %d/%d: a tap lies on a rounding tie" % (p, q))
        row = [int(math.floor(x + 0.5)) for x in v]
        row[max(range(t), key=lambda n: (v[n], -n))] += 65536 - sum(row)
        h[phi] = row
    if (int(np.abs(h.astype(np.int64)).sum(axis=1).max()) * 8192) >> 16 >= 32768:
        raise RateError("rate %d/%d: the int16 store could wrap" % (p, q))
    return h


def permitted_blocks(q: int) -> int:
    """Submits carry a multiple of this many blocks: Q / gcd(Q, 64), the odd part of a Q <= 64.  A submit then holds
    k * P * 512 * (64 / gcd(Q, 64)) input samples: a whole number of 512-sample windows.  (The odd part alone would not do at
    Q = 128: one block of 129/128 is 33024 samples, 64.5 windows.)"""
    q = int(q)
    return q // math.gcd(q, 64)


def input_samples(n_blocks: int, p: int, q: int) -> int:
    """Complex input samples a submit of n_blocks blocks consumes per stream; RateError unless n_blocks is a multiple of
    permitted_blocks(q)."""
    if n_blocks < 1 or int(n_blocks) % permitted_blocks(q):
        raise RateError("%d blocks at %d/%d: a submit holds a multiple of %d blocks" % (n_blocks, p, q, permitted_blocks(q)))
    return int(n_blocks) * 32768 * int(p) // int(q)


def resample_x16(x16, p: int, q: int, hist=None) -> np.ndarray:
    """The stage on int16 input (what the input-rate tune feeds it): interleaved int16 (I, Q) at 1536000 P / Q ->
    interleaved int16 (I, Q) at 1.536 MS/s.  The whole input as one stream from zero history (hist = None), or -- the input of a
    submit that follows a permitted boundary -- from `hist`, the (at least T - 1) int16 complex samples before it
    (interleaved); phase 0 falls on the first sample either way."""
    h = taps(p, q).astype(np.int64)
    t = h.shape[1]
    x = np.ascontiguousarray(x16, dtype=np.int16).reshape(-1, 2).astype(np.int64)
    n_in = len(x)
    lead = np.zeros((t - 1, 2), dtype=np.int64)
    if hist is not None:
        hr = np.ascontiguousarray(hist, dtype=np.int16).reshape(-1, 2)
        assert len(hr) >= t - 1
        lead = hr[len(hr) - (t - 1):].astype(np.int64)
    xp = np.concatenate([lead, x])  # xp[k] = x[k - (T - 1)]
    n_out = (n_in * q + p - 1) // p  # outputs whose newest sample i0 lies inside the input
    out = np.empty((n_out, 2), dtype=np.int16)
    step = 1 << 16
    for m0 in range(0, n_out, step):
        a = np.arange(m0, min(n_out, m0 + step), dtype=np.int64) * p
        i0, phi = a // q, a % q
        idx = i0[:, None] + np.arange(t, dtype=np.int64)[None, :]
        hh = h[phi]
        for rail in range(2):
            acc = ((xp[idx, rail] * hh) >> 16).sum(axis=1)
            out[m0:m0 + len(a), rail] = acc.astype(np.int16)  # (never wraps: taps() refuses a rate where it could)
    return out.reshape(-1)


def _widen(iq_u8) -> np.ndarray:
    return ((np.ascontiguousarray(iq_u8, dtype=np.uint8).astype(np.int16) - 128) << 6).astype(np.int16)


def resample_s16(iq_u8, p: int, q: int, hist=None) -> np.ndarray:
    """u8 IQ (interleaved) at 1536000 P / Q -> interleaved int16 (I, Q) at 1.536 MS/s: the whole input as one stream from
    zero history (hist = None), or -- the input of a submit that follows a permitted boundary -- from `hist`, the (at least
    T - 1) raw u8 complex samples before it (interleaved); phase 0 falls on the first sample either way."""
    return resample_x16(_widen(iq_u8), p, q, None if hist is None else _widen(hist))


def abs_sum_max(p: int, q: int) -> int:
    """max_phi sum_n |h[phi][n]|: what bounds |y0|.  The input-rate tune (6g) is refused where this * 11585 >> 16 >= 32768."""
    return int(np.abs(taps(p, q).astype(np.int64)).sum(axis=1).max())
