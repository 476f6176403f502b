"""The burst envelope (tfrec_amd_enable_burst_envelope, include/tfrec_amd.h: tfrec_amd_envelope) restated in numpy -- no
GPU needed.  Written from the header's definition alone; exact integers throughout.

Per run of the recorder's table: how many of its samples are over the threshold and where the last of them lies, the gaps between
them, and the energy and the burst meter's product sums split at that last over sample into head (the burst) and tail (the
trigger's hold: the burst's own noise reference).

  thresholds            the threshold in force at every sample of one stream (levels.py's recurrence, auto streams included);
  envelopes             vectorised, from the definition: one submit's records from every stream's decimated samples, its over bits
                        (or the thresholds that give them), its run table and the pair ahead of every stream's first sample;
  envelopes_bruteforce  the same sample by sample, in Python integers;
  merge                 a chain of pieces -> the record of the uncut run;  chains: the chains of a sequence of submits
                        (burst.chains' walk);  split: a record's run cut into pieces at given samples (the per-block form: the
                        pieces merge back into the record, which is how a gap across a block boundary is specified);
  summary               burst length, tail length, ratio_c and snr_db of a merged record;  line: tfrec_gpu -Q's output line.
"""
from __future__ import annotations

import math

import numpy as np

from . import burst, levels
from .capture import RUN_CONTINUES, RUN_OPEN

ENVELOPE_DTYPE = np.dtype([("stream", "<u4"), ("flags", "<u4"), ("start_sample", "<i8"), ("n_samples", "<u4"), ("thresh", "<i4"),
                           ("n_over", "<u4"), ("last_over", "<i4"), ("energy_head", "<u8"), ("energy_tail", "<u8"),
                           ("n_gaps", "<u4"), ("max_gap", "<u4"), ("lead_not_over", "<u4"), ("nprod_head", "<u4"),
                           ("dot_head", "<i8"), ("crs_head", "<i8"), ("dot_tail", "<i8"), ("crs_tail", "<i8"),
                           ("nprod_tail", "<u4"), ("reserved", "<u4", (7,))])
assert ENVELOPE_DTYPE.itemsize == 128
SPLIT = ("energy", "dot", "crs", "nprod")  # the quantities kept as <name>_head and <name>_tail
MIN_TAIL = 64  # the summary's condition on n_tail


def thresholds(dec, types_mask: int, thresh: int, state: dict | None = None):
    """-> (thr[M], state): the threshold in force at every decimated sample of ONE stream -- per block of 8192 samples the
    level meter's `thresh` (levels.levels: fm_demod.cpp:58-73's recurrence; -t 0: auto) --, and the state that continues the
    stream.  over[n] = |I[n]| + |Q[n]| > thr[n] is the stream's final trigger mask."""
    rec, st = levels.levels(dec, types_mask, thresh, state)
    return np.repeat(rec["thresh"].astype(np.int64), levels.BLOCK_DEC), st


def _over(z, m):
    """One stream's over bits: m is the bits themselves (bool [M]) or the threshold (a number, or one per sample)."""
    m = np.asarray(m)
    if m.dtype == np.bool_:
        assert m.shape == (len(z),)
        return m
    return np.abs(z[:, 0]) + np.abs(z[:, 1]) > m.astype(np.int64)


def _copied(run):
    o = np.zeros((), dtype=ENVELOPE_DTYPE)
    for f in ("stream", "flags", "n_samples", "thresh"):
        o[f] = run[f]
    o["start_sample"] = int(run["start_sample"])
    return o


def _window(dec, mask_or_thresh, r, prev, base, cache):
    s = int(r["stream"])
    if s not in cache:
        z = burst._pairs(dec[s]).astype(np.int64)
        cache[s] = (z, _over(z, mask_or_thresh[s]))
    z, over = cache[s]
    a = int(r["start_sample"]) - (int(base[s]) if base is not None else 0)
    n = int(r["n_samples"])
    assert 0 <= a and a + n <= len(z) and n >= 1
    p = z[a - 1] if a > 0 else np.asarray(prev[s], dtype=np.int64).reshape(2)
    return z[a:a + n], over[a:a + n], p


def envelopes(dec, mask_or_thresh, runs, prev, base=None):
    """One submit's records.  dec[s]: stream s's decimated samples of the submit (int16 pairs, as tfrec_amd_read_decimated returns
    them); mask_or_thresh[s]: its over bits (bool, one per sample) or the threshold behind them (a number, or one per sample:
    thresholds()); runs: the submit's table (RUN_DTYPE, or any records with its first five fields); prev[s]: the pair ahead of the
    submit's first sample; base[s]: the start_sample of the submit's first sample of stream s (default 0) -> an ENVELOPE_DTYPE
    array, one record per table entry."""
    out = np.zeros(len(runs), dtype=ENVELOPE_DTYPE)
    cache = {}
    for e, r in enumerate(runs):
        z, over, p = _window(dec, mask_or_thresh, r, prev, base, cache)
        n = len(z)
        o = _copied(r)
        idx = np.flatnonzero(over)
        last = int(idx[-1]) if len(idx) else -1
        o["n_over"], o["last_over"] = len(idx), last
        o["lead_not_over"] = int(idx[0]) if len(idx) else n
        d = np.diff(idx) - 1  # the not-over samples between consecutive over samples
        d = d[d > 0]
        o["n_gaps"], o["max_gap"] = len(d), int(d.max()) if len(d) else 0
        I, Q = z[:, 0], z[:, 1]
        en = I * I + Q * Q
        o["energy_head"], o["energy_tail"] = int(en[:last + 1].sum()), int(en[last + 1:].sum())
        k0 = 0 if int(r["flags"]) & RUN_CONTINUES else 1
        Ip, Qp = np.concatenate([[p[0]], I[:-1]])[k0:], np.concatenate([[p[1]], Q[:-1]])[k0:]
        dot = I[k0:] * Ip + Q[k0:] * Qp
        crs = Q[k0:] * Ip - I[k0:] * Qp
        live = (dot != 0) | (crs != 0)
        head = np.arange(k0, n) <= last
        for name, sel in (("head", live & head), ("tail", live & ~head)):
            o["nprod_" + name] = int(np.count_nonzero(sel))
            o["dot_" + name], o["crs_" + name] = int(dot[sel].sum()), int(crs[sel].sum())
        out[e] = o
    return out


def envelopes_bruteforce(dec, mask_or_thresh, runs, prev, base=None):
    """The same, one sample at a time in Python integers: two passes, the first finds last_over."""
    out = np.zeros(len(runs), dtype=ENVELOPE_DTYPE)
    cache = {}
    for e, r in enumerate(runs):
        z, over, p = _window(dec, mask_or_thresh, r, prev, base, cache)
        z, over, p = z.tolist(), over.tolist(), [int(v) for v in p]
        n = len(z)
        cont = bool(int(r["flags"]) & RUN_CONTINUES)
        last = -1
        for k in range(n):
            if over[k]:
                last = k
        n_over = n_gaps = max_gap = 0
        lead, stretch, seen = n, 0, False
        v = dict.fromkeys([a + "_" + b for a in SPLIT for b in ("head", "tail")], 0)
        for k in range(n):
            i, q = z[k]
            part = "head" if k <= last else "tail"
            v["energy_" + part] += i * i + q * q
            if over[k]:
                n_over += 1
                if not seen:
                    lead = k
                elif stretch:
                    n_gaps += 1
                    max_gap = max(max_gap, stretch)
                seen, stretch = True, 0
            else:
                stretch += 1
            if k == 0 and not cont:
                continue
            ip, qp = z[k - 1] if k > 0 else p
            dot, crs = i * ip + q * qp, q * ip - i * qp
            if dot == 0 and crs == 0:
                continue
            v["nprod_" + part] += 1
            v["dot_" + part] += dot
            v["crs_" + part] += crs
        o = _copied(r)
        o["n_over"], o["last_over"], o["n_gaps"], o["max_gap"], o["lead_not_over"] = n_over, last, n_gaps, max_gap, lead
        for f, x in v.items():
            o[f] = x
        out[e] = o
    return out


def merge2(a, b):
    """Piece (or merged chain) a and the piece b that continues it -> the record of the two as one piece (the header's Cutting)."""
    assert b["stream"] == a["stream"] and int(b["flags"]) & RUN_CONTINUES
    o = a.copy()
    na, la, lb = int(a["n_samples"]), int(a["last_over"]), int(b["last_over"])
    o["n_samples"] = na + int(b["n_samples"])
    o["n_over"] = int(a["n_over"]) + int(b["n_over"])
    for q in SPLIT:
        ah, at, bh, bt = (int(x[q + "_" + part]) for x in (a, b) for part in ("head", "tail"))
        if lb >= 0:
            o[q + "_head"], o[q + "_tail"] = ah + at + bh, bt
        else:
            o[q + "_head"], o[q + "_tail"] = ah, at + bh + bt
    o["last_over"] = na + lb if lb >= 0 else la
    o["lead_not_over"] = int(a["lead_not_over"]) if la >= 0 else na + int(b["lead_not_over"])
    joined = (na - 1 - la) + int(b["lead_not_over"])  # the stretch across the cut
    both = la >= 0 and lb >= 0
    o["n_gaps"] = int(a["n_gaps"]) + int(b["n_gaps"]) + (1 if both and joined > 0 else 0)
    o["max_gap"] = max(int(a["max_gap"]), int(b["max_gap"]), joined if both else 0)
    o["flags"] = (int(a["flags"]) & RUN_CONTINUES) | (int(b["flags"]) & RUN_OPEN)
    return o


def merge(pieces):
    """A chain of pieces (in order; piece i + 1 has CONTINUES, piece i OPEN, one stream) -> one record, that of the uncut run."""
    pieces = list(pieces)
    o = pieces[0].copy()
    o["flags"] = int(o["flags"]) & (RUN_CONTINUES | RUN_OPEN)
    for p in pieces[1:]:
        o = merge2(o, p)
    return o


def chains(submits, restarts=None):
    """submits: one ENVELOPE_DTYPE array per submit, in order -> the merged bursts, in burst.chains' order (as they end; a chain
    still open behind the last submit last, by stream).  restarts: {submit index: streams that restart with it}."""
    return burst.chains(submits, restarts, join=merge)


def split(dec, mask_or_thresh, run, prev, cuts, base=None):
    """The per-block form: the run's window cut at the submit-relative samples `cuts` that lie inside it -> the pieces' records,
    as if a submit boundary lay at every cut (the later pieces CONTINUE, the earlier are OPEN).  merge() of them is the run's own
    record: cutting at the block boundaries and merging is how the gaps of a run that spans blocks are defined."""
    s = int(run["stream"])
    a = int(run["start_sample"]) - (int(base[s]) if base is not None else 0)
    n = int(run["n_samples"])
    edges = [a] + sorted(c for c in set(cuts) if a < c < a + n) + [a + n]
    pieces = np.zeros(len(edges) - 1, dtype=ENVELOPE_DTYPE)
    for i in range(len(edges) - 1):
        pieces[i] = _copied(run)
        pieces[i]["start_sample"] = int(run["start_sample"]) + edges[i] - a
        pieces[i]["n_samples"] = edges[i + 1] - edges[i]
        pieces[i]["flags"] = ((int(run["flags"]) & RUN_CONTINUES) if i == 0 else RUN_CONTINUES) | \
            ((int(run["flags"]) & RUN_OPEN) if i == len(edges) - 2 else RUN_OPEN)
    return envelopes(dec, mask_or_thresh, pieces, prev, base)


def summary(rec):
    """-> (burst_samples, n_tail, ratio_c, snr_db) of a merged record: len = last_over + 1, n_tail = n_samples - len, ratio_c =
    floor(100 energy_head n_tail / (energy_tail len)) -- None unless the chain is not OPEN, len > 0, energy_tail > 0 and n_tail
    >= 64 --, snr_db = 10 log10(ratio_c / 100), None when ratio_c is None or 0."""
    length = int(rec["last_over"]) + 1
    n_tail = int(rec["n_samples"]) - length
    et = int(rec["energy_tail"])
    ratio = None
    if not int(rec["flags"]) & RUN_OPEN and length > 0 and et > 0 and n_tail >= MIN_TAIL:
        ratio = 100 * int(rec["energy_head"]) * n_tail // (et * length)
    return length, n_tail, ratio, (10.0 * math.log10(ratio / 100.0) if ratio else None)


def line(name: str, rec) -> str:
    """tfrec_gpu -Q: extent <file> <start_sample> <n_samples> <burst_samples> <n_over> <n_gaps> <max_gap> <ratio_c|-> <snr_db|->"""
    length, _, ratio, snr = summary(rec)
    return "extent %s %d %d %d %d %d %d %s %s" % (
        name, int(rec["start_sample"]), int(rec["n_samples"]), length, int(rec["n_over"]), int(rec["n_gaps"]), int(rec["max_gap"]),
        "-" if ratio is None else "%d.%02d" % (ratio // 100, ratio % 100), "-" if snr is None else "%.1f" % snr)
