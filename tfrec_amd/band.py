"""The burst band (tfrec_amd_enable_burst_band, include/tfrec_amd.h: tfrec_amd_band) restated in numpy -- no GPU
needed.  Written from the header's definition alone; exact integers throughout.

Per run of the recorder's table: the summed power spectrum of the burst's own IQ, 256 bins of 750 Hz over -96 .. +95.25 kHz,
Hann-windowed, taken over the 512-sample segments that lie wholly inside the run.  It peaks where the burst's carrier or tones lie,
to a fraction of a bin, and its extent is the burst's occupied bandwidth.

  bands              vectorised, from the definition: one submit's records from every stream's decimated samples and its run table;
  bands_bruteforce   the same sample by sample and bin by bin, in Python integers;
  merge              a chain of pieces -> the record of the uncut run;  chains: the chains of a sequence of submits (burst.chains' walk);
  summary            peak_hz, centre_hz, bw_hz, lo_hz and hi_hz of a merged record;  line: tfrec_gpu -I's output line.
"""
from __future__ import annotations

import numpy as np

from . import burst, tune
from .capture import RUN_CONTINUES, RUN_OPEN
from .clock import SPEC_MAX, SUMMED, _window

SEG = 512  # samples per segment
N_BINS = 256
BIN0 = -128  # spec[i] is bin j = BIN0 + i
BIN_HZ = 750  # 384000 / 512
X_SHIFT = 14  # P = (X_re >> 14)^2 + (X_im >> 14)^2
BAND_DTYPE = np.dtype([("stream", "<u4"), ("flags", "<u4"), ("start_sample", "<i8"), ("n_samples", "<u4"), ("thresh", "<i4"),
                       ("n_segments", "<u4"), ("n_silent", "<u4"), ("spec", "<u8", (N_BINS,))])
assert BAND_DTYPE.itemsize == 2080


def window():
    """Wn[m'] = 32767 - C[(8 m') mod 4096], m' = 0 .. 511: a Hann window, 0 at m' = 0 and 65534 at m' = 256 (int64)."""
    c, _ = tune.table()
    return 32767 - c.astype(np.int64)[(8 * np.arange(SEG)) % (1 << tune.TABLE_BITS)]


def _tables():
    """C[(8 j m') & 4095] and S[...] as int64 [256, 512], row j + 128."""
    c, s = tune.table()
    t = (8 * np.arange(BIN0, BIN0 + N_BINS)[:, None] * np.arange(SEG)[None, :]) & ((1 << tune.TABLE_BITS) - 1)
    return c.astype(np.int64)[t], s.astype(np.int64)[t]


_WN = window()
_CM, _SM = _tables()


def _copied(run):
    o = np.zeros((), dtype=BAND_DTYPE)
    for f in ("stream", "flags", "n_samples", "thresh"):
        o[f] = run[f]
    o["start_sample"] = int(run["start_sample"])
    return o


def windowed(z):
    """One segment's 512 pairs (int64 [512, 2]) -> its windowed samples (wI, wQ) as int64 [512, 2], or None for a silent segment."""
    mx = int(np.abs(z).max())
    if mx == 0:
        return None
    x = z >> max(0, mx.bit_length() - 13)
    return (x * _WN[:, None]) >> 16


def bands(dec, runs, base=None):
    """One submit's records.  dec[s]: stream s's decimated samples of the submit (int16 pairs, as tfrec_amd_read_decimated returns
    them; a whole number of 8192-sample blocks); runs: the submit's table (RUN_DTYPE, or any records with its first five fields);
    base[s]: the start_sample of the submit's first sample of stream s (default 0) -> a BAND_DTYPE array, one per table entry."""
    out = np.zeros(len(runs), dtype=BAND_DTYPE)
    for e, r in enumerate(runs):
        s, a, n = _window(dec, r, base)
        z = burst._pairs(dec[s]).astype(np.int64)
        o = _copied(r)
        rows = []
        for q in range(-(-a // SEG), (a + n) // SEG):
            w = windowed(z[SEG * q:SEG * q + SEG])
            if w is None:
                o["n_silent"] += 1
            else:
                rows.append(w)
        o["n_segments"] = len(rows)
        if rows:
            W = np.array(rows, dtype=np.int64)
            wi, wq = W[:, :, 0], W[:, :, 1]
            xr, xi = (wi @ _CM.T + wq @ _SM.T) >> X_SHIFT, (wq @ _CM.T - wi @ _SM.T) >> X_SHIFT  # |X| < 2^38: exact in int64
            o["spec"] = (xr * xr + xi * xi).sum(axis=0).astype(np.uint64)  # (< 2^49 each: exact below 2^15 segments)
        out[e] = o
    return out


def bands_bruteforce(dec, runs, base=None):
    """The same, one sample and one bin at a time in Python integers."""
    c, s_ = tune.table()
    C, S = [int(v) for v in c], [int(v) for v in s_]
    out = np.zeros(len(runs), dtype=BAND_DTYPE)
    for e, r in enumerate(runs):
        s, a, n = _window(dec, r, base)
        z = burst._pairs(dec[s]).tolist()
        nseg = nsil = 0
        spec = [0] * N_BINS
        for q in range(len(z) // SEG):
            if not (a <= SEG * q and SEG * q + SEG <= a + n):
                continue
            zz = z[SEG * q:SEG * q + SEG]
            mx = max(max(abs(i), abs(k)) for i, k in zz)
            if mx == 0:
                nsil += 1
                continue
            nseg += 1
            sh = max(0, mx.bit_length() - 13)
            w = [(((i >> sh) * (32767 - C[8 * m])) >> 16, ((k >> sh) * (32767 - C[8 * m])) >> 16) for m, (i, k) in enumerate(zz)]
            for b in range(N_BINS):
                j = BIN0 + b
                xr = xi = 0
                for m, (wi, wq) in enumerate(w):
                    t = (8 * j * m) & 4095
                    xr += wi * C[t] + wq * S[t]
                    xi += wq * C[t] - wi * S[t]
                spec[b] += (xr >> X_SHIFT) ** 2 + (xi >> X_SHIFT) ** 2
        o = _copied(r)
        o["n_segments"], o["n_silent"], o["spec"] = nseg, nsil, spec
        out[e] = o
    return out


def merge(pieces):
    """A chain of pieces (in order; piece i + 1 has CONTINUES, piece i OPEN, one stream) -> one record, that of the uncut run: the
    clock's rule -- n_samples, n_segments, n_silent and spec added, spec saturating at 2^64 - 1."""
    pieces = list(pieces)
    o = pieces[0].copy()
    spec = [int(v) for v in o["spec"]]
    for p in pieces[1:]:
        assert p["stream"] == o["stream"] and int(p["flags"]) & RUN_CONTINUES
        for f in SUMMED:
            o[f] = o[f] + p[f]
        spec = [min(v + int(w), SPEC_MAX) for v, w in zip(spec, p["spec"])]
    o["spec"] = np.array(spec, dtype=np.uint64)
    o["flags"] = (int(pieces[0]["flags"]) & RUN_CONTINUES) | (int(pieces[-1]["flags"]) & RUN_OPEN)
    return o


def chains(submits, restarts=None):
    """submits: one BAND_DTYPE array per submit, in order -> the merged bursts, in burst.chains' order."""
    return burst.chains(submits, restarts, join=merge)


def _lowest_max(P, j0, j1):
    """The lowest j of the maximum of P over the bins j0 .. j1."""
    part = P[j0 - BIN0:j1 - BIN0 + 1]
    return j0 + part.index(max(part))


def summary(rec):
    """-> (peak_hz, centre_hz, bw_hz, lo_hz, hi_hz) of a merged record, or None when n_segments == 0 or the spectrum is empty.  P[j]
    = spec[j + 128], tot its sum.  peak_hz = 750 jp + off: jp the lowest j of the maximum, off the clock's parabola in the bin's unit,
    floor((750 num + den) / (2 den)) with num = P[jp+1] - P[jp-1], den = 2 P[jp] - P[jp-1] - P[jp+1], if den > 0 and neither neighbour
    exceeds P[jp], else 0, and 0 at jp = -128 and 127.  centre_hz = floor(750 sum j P[j] / tot).  bw_hz = 750 (hi - lo + 1): lo the
    largest j with 200 * sum_{i<j} P[i] <= tot, hi the smallest j with 200 * sum_{i>j} P[i] <= tot.  lo_hz = 750 jl, hi_hz = 750 jh:
    jl the lowest j of the maximum over j <= c, jh over j > c, c = min(floor(centre_hz / 750), 126)."""
    P = [int(v) for v in rec["spec"]]
    tot = sum(P)
    if int(rec["n_segments"]) == 0 or tot == 0:
        return None
    top = BIN0 + N_BINS - 1
    jp = _lowest_max(P, BIN0, top)
    off = 0
    if BIN0 < jp < top:
        p0, pm, pp = P[jp - BIN0], P[jp - 1 - BIN0], P[jp + 1 - BIN0]
        num, den = pp - pm, 2 * p0 - pm - pp
        if den > 0 and pm <= p0 and pp <= p0:
            off = (BIN_HZ * num + den) // (2 * den)
    centre = BIN_HZ * sum((BIN0 + i) * p for i, p in enumerate(P)) // tot
    lo, below = BIN0, 0
    while 200 * (below + P[lo - BIN0]) <= tot:  # (ends below the top bin: tot > 0)
        below += P[lo - BIN0]
        lo += 1
    hi, above = top, 0
    while 200 * (above + P[hi - BIN0]) <= tot:
        above += P[hi - BIN0]
        hi -= 1
    c = min(centre // BIN_HZ, top - 1)
    return BIN_HZ * jp + off, centre, BIN_HZ * (hi - lo + 1), BIN_HZ * _lowest_max(P, BIN0, c), BIN_HZ * _lowest_max(P, c + 1, top)


def line(name: str, rec) -> str:
    """tfrec_gpu -I: band <file> <start_sample> <n_samples> <n_segments> <peak_hz|-> <centre_hz|-> <bw_hz|-> <lo_hz|-> <hi_hz|->"""
    sm = summary(rec)
    return "band %s %d %d %d %s" % (name, int(rec["start_sample"]), int(rec["n_samples"]), int(rec["n_segments"]),
                                   "- - - - -" if sm is None else "%d %d %d %d %d" % sm)
