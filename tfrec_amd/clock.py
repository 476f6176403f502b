"""The burst clock (tfrec_amd_enable_burst_clock, include/tfrec_amd.h: tfrec_amd_clock) restated in numpy -- no GPU
needed.  Written from the header's definition alone; exact integers throughout.

Per run of the recorder's table: the summed power spectrum, 128 bins of 375 Hz from 1500 Hz, of the real part of the second-order
product of the decimated samples, taken over the 1024-sample segments that lie wholly inside the run.  That signal dips at every
frequency transition, so its spectrum peaks at the symbol rate.

  segments           the g16 rows of the segments of one run (what the spectrum is taken of), and the number of silent ones;
  clocks             vectorised, from the definition: one submit's records from every stream's decimated samples and its run table;
  clocks_bruteforce  the same sample by sample and bin by bin, in Python integers;
  merge              a chain of pieces -> the record of the uncut run;  chains: the chains of a sequence of submits (burst.chains' walk);
  summary            clock_hz and quality_c of a merged record;  line: tfrec_gpu -C's output line.
"""
from __future__ import annotations

import numpy as np

from . import burst, tune
from .capture import RUN_CONTINUES, RUN_OPEN

SEG = 1024  # samples per segment
N_BINS = 128
BIN0 = 4  # spec[i] is bin j = BIN0 + i
BIN_HZ = 375  # 384000 / 1024
BAND = (12, 128)  # the summary's band, inclusive: 4500 .. 48000 Hz
CLOCK_DTYPE = np.dtype([("stream", "<u4"), ("flags", "<u4"), ("start_sample", "<i8"), ("n_samples", "<u4"), ("thresh", "<i4"),
                        ("n_segments", "<u4"), ("n_silent", "<u4"), ("spec", "<u8", (N_BINS,))])
assert CLOCK_DTYPE.itemsize == 1056
SUMMED = ("n_samples", "n_segments", "n_silent")
SPEC_MAX = (1 << 64) - 1


def _tables():
    """C[(4 j m') mod 4096] and S[...] as int64 [128, 1024]."""
    c, s = tune.table()
    k = (4 * np.arange(BIN0, BIN0 + N_BINS)[:, None] * np.arange(SEG)[None, :]) % (1 << tune.TABLE_BITS)
    return c.astype(np.int64)[k], s.astype(np.int64)[k]


_CM, _SM = _tables()


def _copied(run):
    o = np.zeros((), dtype=CLOCK_DTYPE)
    for f in ("stream", "flags", "n_samples", "thresh"):
        o[f] = run[f]
    o["start_sample"] = int(run["start_sample"])
    return o


def _whole(a, n):
    """The submit-relative first samples of the segments wholly inside [a, a + n)."""
    q0 = -(-a // SEG)
    q1 = (a + n) // SEG
    return [SEG * q for q in range(q0, q1)]


def g16_of(z):
    """One segment's 1024 pairs (int64 [1024, 2]) -> its g16 (int64 [1024]), or None for a silent segment."""
    I, Q = z[:, 0], z[:, 1]
    dot = np.zeros(SEG, dtype=np.int64)
    crs = np.zeros(SEG, dtype=np.int64)
    dot[1:] = I[1:] * I[:-1] + Q[1:] * Q[:-1]
    crs[1:] = Q[1:] * I[:-1] - I[1:] * Q[:-1]
    mx = int(max(np.abs(dot).max(), np.abs(crs).max()))
    if mx == 0:
        return None
    sh = max(0, mx.bit_length() - 15)
    d, c = dot >> sh, crs >> sh
    g = np.zeros(SEG, dtype=np.int64)
    g[2:] = d[2:] * d[1:-1] + c[2:] * c[1:-1]
    return np.minimum(g >> 16, 32767)


def segments(dec_s, a, n):
    """Stream samples dec_s, a run at submit-relative [a, a + n) -> (g16 rows of its non-silent whole segments [k, 1024], n_silent)."""
    z = burst._pairs(dec_s)
    rows, silent = [], 0
    for m0 in _whole(a, n):
        g = g16_of(z[m0:m0 + SEG].astype(np.int64))
        if g is None:
            silent += 1
        else:
            rows.append(g)
    return (np.array(rows, dtype=np.int64).reshape(-1, SEG)), silent


def _window(dec, r, base):
    s = int(r["stream"])
    a = int(r["start_sample"]) - (int(base[s]) if base is not None else 0)
    n = int(r["n_samples"])
    assert 0 <= a and a + n <= len(burst._pairs(dec[s])) and n >= 1
    return s, a, n


def clocks(dec, runs, base=None):
    """One submit's records.  dec[s]: stream s's decimated samples of the submit (int16 pairs, as tfrec_amd_read_decimated returns
    them; a whole number of 8192-sample blocks); runs: the submit's table (RUN_DTYPE, or any records with its first five fields);
    base[s]: the start_sample of the submit's first sample of stream s (default 0) -> a CLOCK_DTYPE array, one per table entry."""
    out = np.zeros(len(runs), dtype=CLOCK_DTYPE)
    for e, r in enumerate(runs):
        s, a, n = _window(dec, r, base)
        o = _copied(r)
        G, silent = segments(dec[s], a, n)
        o["n_segments"], o["n_silent"] = len(G), silent
        if len(G):
            xr, xi = (G @ _CM.T) >> 16, (G @ _SM.T) >> 16  # |X| < 2^40: exact in int64
            o["spec"] = (xr * xr + xi * xi).sum(axis=0).astype(np.uint64)  # (< 2^49 each: exact below 2^15 segments)
        out[e] = o
    return out


def clocks_bruteforce(dec, runs, base=None):
    """The same, one sample and one bin at a time in Python integers."""
    c, s_ = tune.table()
    C, S = [int(v) for v in c], [int(v) for v in s_]
    out = np.zeros(len(runs), dtype=CLOCK_DTYPE)
    for e, r in enumerate(runs):
        s, a, n = _window(dec, r, base)
        z = burst._pairs(dec[s]).tolist()
        nseg = nsil = 0
        spec = [0] * N_BINS
        for q in range(len(z) // SEG):
            if not (a <= SEG * q and SEG * q + SEG <= a + n):
                continue
            zz = z[SEG * q:SEG * q + SEG]
            dot, crs = [0] * SEG, [0] * SEG
            for m in range(1, SEG):
                (i, k), (ip, kp) = zz[m], zz[m - 1]
                dot[m], crs[m] = i * ip + k * kp, k * ip - i * kp
            mx = max(max(abs(v) for v in dot), max(abs(v) for v in crs))
            if mx == 0:
                nsil += 1
                continue
            nseg += 1
            sh = max(0, mx.bit_length() - 15)
            d, cc = [v >> sh for v in dot], [v >> sh for v in crs]
            g16 = [0, 0] + [min((d[m] * d[m - 1] + cc[m] * cc[m - 1]) >> 16, 32767) for m in range(2, SEG)]
            for i in range(N_BINS):
                j = BIN0 + i
                xr = xi = 0
                for m in range(2, SEG):
                    if g16[m]:
                        k = (4 * j * m) % 4096
                        xr += g16[m] * C[k]
                        xi += g16[m] * S[k]
                spec[i] += (xr >> 16) ** 2 + (xi >> 16) ** 2
        o = _copied(r)
        o["n_segments"], o["n_silent"], o["spec"] = nseg, nsil, spec
        out[e] = o
    return out


def merge(pieces):
    """A chain of pieces (in order; piece i + 1 has CONTINUES, piece i OPEN, one stream) -> one record, that of the uncut run: the
    first piece's stream, start_sample and thresh, the first piece's CONTINUES and the last one's OPEN, n_samples, n_segments,
    n_silent and spec added, spec saturating at 2^64 - 1."""
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
    """submits: one CLOCK_DTYPE array per submit, in order -> the merged bursts, in burst.chains' order (as they end; a chain still
    open behind the last submit last, by stream).  restarts: {submit index: streams that restart with it}."""
    return burst.chains(submits, restarts, join=merge)


def summary(rec):
    """-> (clock_hz, quality_c) of a merged record, or None when n_segments == 0 or the band is empty.  P[j] = spec[j - 4]; the band
    is j = 12 .. 128; jp the lowest j of its maximum; off = floor((375 num + den) / (2 den)) with num = P[jp+1] - P[jp-1], den =
    2 P[jp] - P[jp-1] - P[jp+1], if den > 0 and neither neighbour exceeds P[jp], else 0; clock_hz = 375 jp + off; quality_c =
    floor(100 * 117 * P[jp] / tot), the peak over the band's mean in hundredths."""
    P = [int(v) for v in rec["spec"]]
    lo, hi = BAND
    band = P[lo - BIN0:hi - BIN0 + 1]
    tot = sum(band)
    if int(rec["n_segments"]) == 0 or tot == 0:
        return None
    jp = lo + band.index(max(band))
    p0, pm, pp = P[jp - BIN0], P[jp - 1 - BIN0], P[jp + 1 - BIN0]
    num, den = pp - pm, 2 * p0 - pm - pp
    off = (BIN_HZ * num + den) // (2 * den) if den > 0 and pm <= p0 and pp <= p0 else 0
    return BIN_HZ * jp + off, 100 * len(band) * p0 // tot


def line(name: str, rec) -> str:
    """tfrec_gpu -C: clock <file> <start_sample> <n_samples> <n_segments> <clock_hz|-> <quality as %d.%02d|->"""
    sm = summary(rec)
    return "clock %s %d %d %d %s %s" % (name, int(rec["start_sample"]), int(rec["n_samples"]), int(rec["n_segments"]),
                                       "-" if sm is None else "%d" % sm[0], "-" if sm is None else "%d.%02d" % (sm[1] // 100, sm[1] % 100))
