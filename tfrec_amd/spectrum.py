"""CPU restatement of the per-input power spectrum (include/tfrec_amd.h: tfrec_amd_enable_spectrum), in exact numpy
int64.  Written from the definition alone: nothing here calls the C library.

    C, S     tune.table(): C[k] = round(32767 cos(2 pi k / 4096)), S[k] = C[(k - 1024) mod 4096];  step = 4096 / N
    window   w[n] = (32767 - C[(n step) mod 4096]) >> 1
    sample   xw = (x w[n] + 2^14) >> 15 per rail
    DFT      t = (k n step) mod 4096:  X_re[k] = sum_n (xwI C[t] + xwQ S[t]),  X_im[k] = sum_n (xwQ C[t] - xwI S[t])
    power    Y = (X + 2^14) >> 15 per component,  p[k] = Y_re^2 + Y_im^2
    records  G consecutive frames: sum[k] = sum p[k], peak[k] = max p[k], n_frames

Every product and sum fits int64 with room to spare (a term < 2^29, |X| < 2^39, p < 2^49, a record's sum < 2^63), so the matrix
product below is exact whatever order numpy sums in.
"""
from __future__ import annotations

import numpy as np

from . import formats, tune

BINS = (64, 128, 256, 512, 1024)
G_MAX = 16384


def _check(n_bins: int, g: int) -> None:
    if n_bins not in BINS:
        raise ValueError("n_bins %r is not one of %r" % (n_bins, BINS))
    if not 1 <= g <= G_MAX:
        raise ValueError("frames_per_record %r outside [1, %d]" % (g, G_MAX))


def window(n_bins: int) -> np.ndarray:
    """w[n], n < N, as int64: the periodic Hann window from the mixer's cosine table."""
    _check(n_bins, 1)
    c, _ = tune.table()
    step = 4096 // n_bins
    return ((32767 - c[(np.arange(n_bins) * step) % 4096].astype(np.int64)) >> 1)


def twiddles(n_bins: int):
    """(C[t], S[t]) for t = (k n step) mod 4096 as int64 matrices [n, k]."""
    _check(n_bins, 1)
    c, s = tune.table()
    step = 4096 // n_bins
    n = np.arange(n_bins, dtype=np.int64)
    t = (np.outer(n, n) * step) % 4096
    return c[t].astype(np.int64), s[t].astype(np.int64)


def frame_power(x_iq_int16, n_bins: int) -> np.ndarray:
    """p[f, k] of every whole frame of a row of x (interleaved int16 I, Q), as uint64 [F, N]."""
    x = np.ascontiguousarray(x_iq_int16, dtype=np.int16).reshape(-1)
    assert x.size % 2 == 0
    nf = (x.size // 2) // n_bins
    w = window(n_bins)
    xi = x[0:2 * nf * n_bins:2].astype(np.int64).reshape(nf, n_bins)
    xq = x[1:2 * nf * n_bins:2].astype(np.int64).reshape(nf, n_bins)
    wi = (xi * w + (1 << 14)) >> 15
    wq = (xq * w + (1 << 14)) >> 15
    ct, st = twiddles(n_bins)
    x_re = wi @ ct + wq @ st
    x_im = wq @ ct - wi @ st
    y_re = (x_re + (1 << 14)) >> 15
    y_im = (x_im + (1 << 14)) >> 15
    return (y_re * y_re + y_im * y_im).astype(np.uint64)


def spectrum(x_iq_int16, n_bins: int, frames_per_record: int, fmt=None):
    """The records of one submit's row -> (sum[n_records, N] uint64, peak[n_records, N] uint64, n_frames[n_records] uint32).
    x_iq_int16: the row as x, interleaved int16 (I, Q) -- or, with fmt ("u8", "s8", "s16", "f32" or a TFREC_AMD_FMT_* number), the
    row's raw bytes, taken through formats.to_x."""
    _check(n_bins, frames_per_record)
    x = formats.to_x(fmt, x_iq_int16) if fmt is not None else x_iq_int16
    p = frame_power(x, n_bins)
    nf = len(p)
    g = int(frames_per_record)
    nr = (nf + g - 1) // g
    s = np.zeros((nr, n_bins), dtype=np.uint64)
    pk = np.zeros((nr, n_bins), dtype=np.uint64)
    cnt = np.zeros(nr, dtype=np.uint32)
    for r in range(nr):
        part = p[r * g:(r + 1) * g]
        s[r] = part.sum(axis=0, dtype=np.uint64)
        pk[r] = part.max(axis=0)
        cnt[r] = len(part)
    return s, pk, cnt


def bin_khz(center_khz: int, fs_in: int, n_bins: int) -> list:
    """The frequency of every bin in kHz as exact fractions of Hz turned to floats: c + (k < N/2 ? k : k - N) fs_in / N, in bin order."""
    return [center_khz + (k if k < n_bins // 2 else k - n_bins) * fs_in / n_bins / 1000.0 for k in range(n_bins)]
