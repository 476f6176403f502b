"""The burst track (tfrec_amd_enable_burst_track, include/tfrec_amd.h: tfrec_amd_track) restated in numpy -- no GPU
needed.  Written from the header's definition alone; exact integers throughout.

Per captured sample of every run of the recorder's table one bit: the sign of a quadrature discriminator about the stream's
centre, boxcar-smoothed over L products -- 1 above the centre --, packed where the sample's pair lies in the pool; per run a
40-byte record.  A run-length slicer turns a merged track and a rate into the burst's bits.  Nothing here has been measured on
real recordings.

  index_of           the table index r of a centre in Hz;
  tracks             vectorised, from the definition: one submit's records and bitmap from every stream's decimated samples, its
                     over bits (or the thresholds that give them), its run table and the state the submit before left;
  tracks_bruteforce  the same sample by sample, in Python integers;
  bits_of            a record's track out of the bitmap;  merge: a chain of pieces -> the record and track of the uncut run;
  chains             the chains of a sequence of submits (burst.chains' walk);
  slice_bits         a track and a rate -> the symbols;  line: tfrec_gpu -G's output line;
  device_bytes, pinned_bytes   what tfrec_amd_enable_burst_track adds to tfrec_amd_get_memory.

The track's amplitude mode (tfrec_amd_enable_burst_track_amplitude, the header's "Amplitude track") -- the same
records, bitmap and state, the bit 1 where the sum of L powers |I| + |Q| lies above L times the stream's level:

  amplitude_tracks, amplitude_tracks_bruteforce   tracks' and tracks_bruteforce's counterparts, a level per stream for the centre;
  pulses             a merged track -> the widths pulse, gap, ..., pulse;  pulses_line: tfrec_gpu -O's output line.

The track's auto-centre mode (tfrec_amd_enable_burst_track_auto, the header's "Auto-centre track") -- the same track
about a table index per ENTRY, measured on the first K samples of the chain's first piece:

  head_centres, head_centres_bruteforce   one submit's centre records (CENTRE_DTYPE) and the carried state, vectorised and per sample;
  auto_tracks        the centre records, then tracks(..., run_index=...) about them;
  merge_centres, centre_chains   a chain keeps its first piece's record;  centre_line: tfrec_gpu -G rate,auto's output line;
  auto_device_bytes  what tfrec_amd_enable_burst_track_auto adds to tfrec_amd_get_memory (pinned: pinned_bytes).

The track's phase mode (tfrec_amd_enable_burst_track_phase, the header's "Phase track") -- the same records, bitmap
and centre records, for phase-keyed bursts: a differential phase detector at a lag of m samples about the carrier measured on
the first K samples of the chain's first piece:

  carrier_index, carrier_index_bruteforce   the search over the 4096 table directions for the sums A, B of a head's products;
  head_carriers, head_carriers_bruteforce   one submit's carrier records (CENTRE_DTYPE) and the carried state;
  phase_tracks, phase_tracks_bruteforce     the carrier records, then the detector about them; fresh_phase_state: the 80 pairs;
  lag_of             tfrec_gpu -G rate,psk's m;  phase_device_bytes: what the enable call adds to tfrec_amd_get_memory.
"""
from __future__ import annotations

import numpy as np

from . import burst, envelope, tune
from .capture import RUN_CONTINUES, RUN_OPEN

AHEAD = 16  # the pairs carried from submit to submit, and the largest L
CENTRE_MAX = 192000
KEEP = 1 << 20  # the samples of a chain's track the host keeps
TRACK_DTYPE = np.dtype([("stream", "<u4"), ("flags", "<u4"), ("start_sample", "<i8"), ("n_samples", "<u4"), ("thresh", "<i4"),
                        ("bit_offset", "<u8"), ("last_over", "<i4"), ("n_ones", "<u4")])
assert TRACK_DTYPE.itemsize == 40


def index_of(hz: int) -> int:
    """r = floor((8192 hz + 384000) / 768000) mod 4096 (Python's // is a true floor)."""
    hz = int(hz)
    if abs(hz) > CENTRE_MAX:
        raise ValueError("centre %d Hz outside [-%d, %d]" % (hz, CENTRE_MAX, CENTRE_MAX))
    return (8192 * hz + 384000) // 768000 % 4096


def fresh_state(n_streams: int) -> dict:
    """What a context carries before its first submit: no pairs, no chain."""
    return {"carry": np.zeros((n_streams, AHEAD, 2), dtype=np.int16), "prior": np.zeros(n_streams, dtype=np.int64)}


def _copied(run):
    o = np.zeros((), dtype=TRACK_DTYPE)
    for f in ("stream", "flags", "n_samples", "thresh"):
        o[f] = run[f]
    o["start_sample"] = int(run["start_sample"])
    o["bit_offset"] = int(run["pool_offset"])
    return o


def _window(dec, r, base):
    s = int(r["stream"])
    a = int(r["start_sample"]) - (int(base[s]) if base is not None else 0)
    n = int(r["n_samples"])
    assert 0 <= a and a + n <= len(burst._pairs(dec[s])) and n >= 1
    cont = bool(int(r["flags"]) & RUN_CONTINUES)
    assert not cont or a == 0
    return s, a, n, cont


def _next_state(dec, runs, state, base):
    """The state behind the submit: every stream's last 16 pairs, and prior = min(16, prior' + n) of the stream's OPEN run."""
    nxt = {"carry": np.array([burst._pairs(d)[-AHEAD:] for d in dec], dtype=np.int16), "prior": np.zeros(len(dec), dtype=np.int64)}
    for r in runs:
        if int(r["flags"]) & RUN_OPEN:
            s = int(r["stream"])
            before = int(state["prior"][s]) if int(r["flags"]) & RUN_CONTINUES else 0
            nxt["prior"][s] = min(AHEAD, before + int(r["n_samples"]))
    return nxt


def _pack(out, tr, max_samples):
    """The runs' tracks -> the bitmap: t[k] at bit bit_offset + k; a run whose samples do not fit max_samples leaves no bit."""
    ends = [int(o["bit_offset"]) + int(o["n_samples"]) for o in out]
    fit = [max_samples is None or e <= max_samples for e in ends]
    total = max([e for e, f in zip(ends, fit) if f], default=0)
    flat = np.zeros(((total + 31) // 32) * 32, dtype=np.uint8)
    for o, t, f in zip(out, tr, fit):
        if f:
            flat[int(o["bit_offset"]):int(o["bit_offset"]) + len(t)] = t
    return np.packbits(flat.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)


class _Rows:
    """Per stream and per call, computed once however many entries the stream has: its pairs as int64, its over bits, and the
    pairs behind the carried ones."""

    def __init__(self, dec, mask_or_thresh, carry=None):
        self.dec, self.mot, self.carry, self.z, self.ov, self.ex = dec, mask_or_thresh, carry, {}, {}, {}

    def pairs(self, s):
        if s not in self.z:
            self.z[s] = burst._pairs(self.dec[s]).astype(np.int64)
        return self.z[s]

    def over(self, s):
        if s not in self.ov:
            self.ov[s] = envelope._over(self.pairs(s), self.mot[s])
        return self.ov[s]

    def extended(self, s):
        if s not in self.ex:
            self.ex[s] = np.concatenate([np.asarray(self.carry[s], dtype=np.int64).reshape(-1, 2), self.pairs(s)])
        return self.ex[s]


def tracks(dec, mask_or_thresh, runs, smooth, centres=None, state=None, base=None, max_samples=None, run_index=None):
    """One submit.  dec[s]: stream s's decimated samples of the submit (int16 pairs, as tfrec_amd_read_decimated returns them);
    mask_or_thresh[s]: its over bits or the threshold behind them (envelope.envelopes'); runs: the submit's table (RUN_DTYPE);
    smooth: L; centres[s]: the stream's centre in Hz (default 0); state: what the submit before returned (default: a fresh
    context's); base[s]: the start_sample of the submit's first sample of stream s (default 0); max_samples: the pool's size
    (default: everything fits); run_index[e]: entry e's own table index r in the stream's centre's place (the auto-centre track:
    head_centres' records' index) -> (a TRACK_DTYPE array, one record per table entry; the bitmap's uint32 words, as many as the
    pairs that fit need; the state behind the submit)."""
    L = int(smooth)
    assert 1 <= L <= AHEAD
    state = fresh_state(len(dec)) if state is None else state
    c, s_ = tune.table()
    out = np.zeros(len(runs), dtype=TRACK_DTYPE)
    tr = []
    rows = _Rows(dec, mask_or_thresh, state["carry"])
    for e, r in enumerate(runs):
        s, a, n, cont = _window(dec, r, base)
        ri = int(run_index[e]) if run_index is not None else index_of(centres[s]) if centres is not None else 0
        C, S = int(c[ri]), int(s_[ri])
        z = rows.extended(s)
        cf = a - (int(state["prior"][s]) if cont else 0)  # the chain's first sample, submit-relative
        m = np.arange(a - (AHEAD - 1), a + n)  # every sample a product may be needed of; z's index is m + 16
        I, Q, Ip, Qp = z[m + AHEAD, 0], z[m + AHEAD, 1], z[m + AHEAD - 1, 0], z[m + AHEAD - 1, 1]
        v = np.where(m > cf, (Q * Ip - I * Qp) * C - (I * Ip + Q * Qp) * S, 0)  # (|v| < 2^47)
        cs = np.concatenate([[0], np.cumsum(v)])
        p = np.arange(n) + AHEAD  # sample a + k is v[k + 15]: the sum of v[k + 16 - L .. k + 15]
        t = (cs[p] - cs[p - L]) > 0
        o = _copied(r)
        over = rows.over(s)[a:a + n]
        idx = np.flatnonzero(over)
        o["last_over"] = int(idx[-1]) if len(idx) else -1
        o["n_ones"] = int(np.count_nonzero(t))
        out[e] = o
        tr.append(t.astype(np.uint8))
    return out, _pack(out, tr, max_samples), _next_state(dec, runs, state, base)


def tracks_bruteforce(dec, mask_or_thresh, runs, smooth, centres=None, state=None, base=None, max_samples=None, run_index=None):
    """The same, one sample at a time in Python integers, as the header words it: the sum of v[k - i] over i < min(L, k + prior)."""
    L = int(smooth)
    state = fresh_state(len(dec)) if state is None else state
    c, s_ = tune.table()
    out = np.zeros(len(runs), dtype=TRACK_DTYPE)
    tr = []
    for e, r in enumerate(runs):
        s, a, n, cont = _window(dec, r, base)
        ri = int(run_index[e]) if run_index is not None else index_of(centres[s]) if centres is not None else 0
        C, S = int(c[ri]), int(s_[ri])
        row = burst._pairs(dec[s]).tolist()
        ahead = np.asarray(state["carry"][s]).reshape(AHEAD, 2).tolist()
        prior = int(state["prior"][s]) if cont else 0
        over = envelope._over(burst._pairs(dec[s]).astype(np.int64), mask_or_thresh[s]).tolist()

        def z(k):  # run-relative; k < 0 only in a CONTINUES run, whose a == 0
            return row[a + k] if a + k >= 0 else ahead[AHEAD + a + k]

        def v(k):
            if k == -prior:  # the chain's first sample
                return 0
            (i, q), (ip, qp) = z(k), z(k - 1)
            return (q * ip - i * qp) * C - (i * ip + q * qp) * S

        t, last = [], -1
        for k in range(n):
            total = 0
            for i in range(min(L, k + prior)):
                total += v(k - i)
            t.append(1 if total > 0 else 0)
            if over[a + k]:
                last = k
        o = _copied(r)
        o["last_over"], o["n_ones"] = last, sum(t)
        out[e] = o
        tr.append(np.array(t, dtype=np.uint8))
    return out, _pack(out, tr, max_samples), _next_state(dec, runs, state, base)


LEVEL_MAX = 65535
PULSES_LISTED = 64  # the pulses tfrec_gpu -O lists


def _levels(levels, n_streams):
    lv = [0] * n_streams if levels is None else [int(x) for x in levels]
    assert len(lv) == n_streams and all(0 <= x <= LEVEL_MAX for x in lv)
    return lv


def amplitude_tracks(dec, mask_or_thresh, runs, smooth, levels=None, state=None, base=None, max_samples=None):
    """One submit of the amplitude track: tracks' inputs, outputs and carried state, with levels[s] (0 .. 65535, default 0), the
    stream's level, in the centres' place."""
    L = int(smooth)
    assert 1 <= L <= AHEAD
    state = fresh_state(len(dec)) if state is None else state
    lv = _levels(levels, len(dec))
    out = np.zeros(len(runs), dtype=TRACK_DTYPE)
    tr = []
    rows = _Rows(dec, mask_or_thresh, state["carry"])
    for e, r in enumerate(runs):
        s, a, n, cont = _window(dec, r, base)
        z = rows.extended(s)
        cf = a - (int(state["prior"][s]) if cont else 0)  # the chain's first sample, submit-relative
        m = np.arange(a - (AHEAD - 1), a + n)  # every sample a power may be needed of; z's index is m + 16
        p = np.where(m >= cf, np.abs(z[m + AHEAD, 0]) + np.abs(z[m + AHEAD, 1]), 0)  # (<= 65536)
        cs = np.concatenate([[0], np.cumsum(p)])
        q = np.arange(n) + AHEAD  # sample a + k is p[k + 15]: the sum of p[k + 16 - L .. k + 15]
        t = (cs[q] - cs[q - L]) > L * lv[s]
        o = _copied(r)
        over = rows.over(s)[a:a + n]
        idx = np.flatnonzero(over)
        o["last_over"] = int(idx[-1]) if len(idx) else -1
        o["n_ones"] = int(np.count_nonzero(t))
        out[e] = o
        tr.append(t.astype(np.uint8))
    return out, _pack(out, tr, max_samples), _next_state(dec, runs, state, base)


def amplitude_tracks_bruteforce(dec, mask_or_thresh, runs, smooth, levels=None, state=None, base=None, max_samples=None):
    """The same, one sample at a time in Python integers, as the header words it: t[k] = 1 iff the sum of p[k - i] over
    0 <= i < L with k - i >= -prior is greater than L * level."""
    L = int(smooth)
    state = fresh_state(len(dec)) if state is None else state
    lv = _levels(levels, len(dec))
    out = np.zeros(len(runs), dtype=TRACK_DTYPE)
    tr = []
    for e, r in enumerate(runs):
        s, a, n, cont = _window(dec, r, base)
        row = burst._pairs(dec[s]).tolist()
        ahead = np.asarray(state["carry"][s]).reshape(AHEAD, 2).tolist()
        prior = int(state["prior"][s]) if cont else 0
        over = envelope._over(burst._pairs(dec[s]).astype(np.int64), mask_or_thresh[s]).tolist()

        def p(k):  # run-relative; k < 0 only in a CONTINUES run, whose a == 0
            i, q = row[a + k] if a + k >= 0 else ahead[AHEAD + a + k]
            return abs(i) + abs(q)

        t, last = [], -1
        for k in range(n):
            total = 0
            for i in range(L):
                if k - i >= -prior:
                    total += p(k - i)
            t.append(1 if total > L * lv[s] else 0)
            if over[a + k]:
                last = k
        o = _copied(r)
        o["last_over"], o["n_ones"] = last, sum(t)
        out[e] = o
        tr.append(np.array(t, dtype=np.uint8))
    return out, _pack(out, tr, max_samples), _next_state(dec, runs, state, base)


def pulses(bits) -> list:
    """The header's Pulses: the maximal runs of equal value of a track (already cut to its first last_over + 1 samples), less a
    leading and a trailing run of zeros -> [pulse, gap, pulse, ..., pulse] in samples ([]: no pulse)."""
    b = np.asarray(bits, dtype=np.uint8)
    on = np.flatnonzero(b)
    if len(on) == 0:
        return []
    b = b[on[0]:on[-1] + 1]
    edges = np.flatnonzero(np.diff(b)) + 1
    return np.diff(np.concatenate([[0], edges, [len(b)]])).tolist()


def pulses_line(name: str, piece) -> str:
    """tfrec_gpu -O: pulses <file> <start_sample> <n_samples> <burst_samples> <n_pulses>[+] <w0,g0,w1,...|->: the pulses of the
    track's first burst_samples = last_over + 1 samples, of the first 2^20 at most; the first 64 pulses are listed (with the gaps
    between them), a + behind n_pulses marks more."""
    rec = piece.rec
    length = int(rec["last_over"]) + 1
    w = pulses(piece.bits[:KEEP][:length])
    n = (len(w) + 1) // 2
    shown = w[:2 * PULSES_LISTED - 1]
    return "pulses %s %d %d %d %d%s %s" % (name, int(rec["start_sample"]), int(rec["n_samples"]), length, min(n, PULSES_LISTED),
                                           "+" if n > PULSES_LISTED else "", ",".join("%d" % x for x in shown) if shown else "-")


# ---- the auto-centre track (tfrec_amd_enable_burst_track_auto, the header's "Auto-centre track")
CENTRE_DTYPE = np.dtype([("stream", "<u4"), ("flags", "<u4"), ("start_sample", "<i8"), ("n_samples", "<u4"), ("thresh", "<i4"),
                         ("n_counted", "<u4"), ("source", "<u4"), ("centre_hz", "<i4"), ("deviation_hz", "<i4"), ("index", "<i4"),
                         ("reserved", "<u4")])
assert CENTRE_DTYPE.itemsize == 48
MEASURED, FALLBACK, INHERITED = 0, 1, 2  # a centre record's source
HEAD_MIN, HEAD_MAX = 64, 4096  # K
COUNT_MIN = 64  # the counted products a measured centre needs


def fresh_centre_state(n_streams: int) -> dict:
    """What a context carries before its first submit, and for a stream without an OPEN run that has a record: nothing (index -1)."""
    return {"index": np.full(n_streams, -1, dtype=np.int64), "centre_hz": np.zeros(n_streams, dtype=np.int64)}


def _centre_copied(run):
    o = np.zeros((), dtype=CENTRE_DTYPE)
    for f in ("stream", "flags", "n_samples", "thresh"):
        o[f] = run[f]
    o["start_sample"] = int(run["start_sample"])
    return o


def _fallbacks(fallback, n_streams):
    fb = [0] * n_streams if fallback is None else [int(x) for x in fallback]
    assert len(fb) == n_streams and all(abs(x) <= CENTRE_MAX for x in fb)
    return fb


def _next_centre_state(n_streams, out):
    nxt = fresh_centre_state(n_streams)
    for o in out:
        if int(o["flags"]) & RUN_OPEN:
            nxt["index"][int(o["stream"])], nxt["centre_hz"][int(o["stream"])] = int(o["index"]), int(o["centre_hz"])
    return nxt


def head_centres(dec, mask_or_thresh, runs, head, fallback=None, state=None, base=None):
    """One submit's centre records.  tracks' dec, mask_or_thresh, runs and base; head: K; fallback[s]: the stream's set centre in Hz
    (default 0); state: what the submit before returned (default: a fresh context's).  runs holds the entries that have a record
    (those below max_runs): an OPEN run that is not among them leaves nothing behind -> (a CENTRE_DTYPE array, one record per
    entry; the state behind the submit: per stream the index and centre of its OPEN run, index -1 without one)."""
    K = int(head)
    assert HEAD_MIN <= K <= HEAD_MAX
    state = fresh_centre_state(len(dec)) if state is None else state
    fb = _fallbacks(fallback, len(dec))
    out = np.zeros(len(runs), dtype=CENTRE_DTYPE)
    rows = _Rows(dec, mask_or_thresh)
    sign = np.where(np.arange(burst.N_BINS) < burst.N_BINS // 2, np.arange(burst.N_BINS), np.arange(burst.N_BINS) - burst.N_BINS)
    for e, r in enumerate(runs):
        s, a, n, cont = _window(dec, r, base)
        o = _centre_copied(r)
        if cont:
            if int(state["index"][s]) >= 0:
                o["source"], o["centre_hz"], o["index"] = INHERITED, int(state["centre_hz"][s]), int(state["index"][s])
            else:
                o["source"], o["centre_hz"], o["index"] = FALLBACK, fb[s], index_of(fb[s])
            out[e] = o
            continue
        nh = min(n, K)
        over = rows.over(s)[a:a + nh]
        z = rows.pairs(s)[a:a + nh]
        I, Q, Ip, Qp = z[1:, 0], z[1:, 1], z[:-1, 0], z[:-1, 1]
        both = over[1:] & over[:-1]
        dot, crs = (I * Ip + Q * Qp)[both], (Q * Ip - I * Qp)[both]
        P = len(dot)
        hist = np.bincount(burst._bins(dot, crs), minlength=burst.N_BINS) if P else np.zeros(burst.N_BINS, dtype=np.int64)
        occ = sign[hist >= (P + 15) // 16] if P >= COUNT_MIN else sign[:0]
        o["n_counted"] = P
        if len(occ):
            lo, hi = int(occ.min()), int(occ.max())
            o["source"], o["centre_hz"], o["deviation_hz"] = MEASURED, 3000 * (lo + hi), 3000 * (hi - lo)
        else:
            o["source"], o["centre_hz"] = FALLBACK, fb[s]
        o["index"] = index_of(int(o["centre_hz"]))
        out[e] = o
    return out, _next_centre_state(len(dec), out)


def head_centres_bruteforce(dec, mask_or_thresh, runs, head, fallback=None, state=None, base=None):
    """The same, one sample at a time in Python integers, as the header words it."""
    K = int(head)
    state = fresh_centre_state(len(dec)) if state is None else state
    fb = _fallbacks(fallback, len(dec))
    out = np.zeros(len(runs), dtype=CENTRE_DTYPE)
    for e, r in enumerate(runs):
        s, a, n, cont = _window(dec, r, base)
        o = _centre_copied(r)
        if cont:
            idx = int(state["index"][s])
            src, hz, dev, cnt = (INHERITED, int(state["centre_hz"][s]), 0, 0) if idx >= 0 else (FALLBACK, fb[s], 0, 0)
            idx = idx if idx >= 0 else index_of(hz)
        else:
            row = burst._pairs(dec[s]).tolist()
            over = envelope._over(burst._pairs(dec[s]).astype(np.int64), mask_or_thresh[s]).tolist()
            hist, cnt = [0] * burst.N_BINS, 0
            for k in range(1, min(n, K)):
                if over[a + k] and over[a + k - 1]:
                    (i, q), (ip, qp) = row[a + k], row[a + k - 1]
                    hist[burst.bin_of(i * ip + q * qp, q * ip - i * qp)] += 1
                    cnt += 1
            occ = [burst.signed_bin(j) for j in range(burst.N_BINS) if cnt >= COUNT_MIN and hist[j] >= (cnt + 15) // 16]
            if occ:
                src, hz, dev = MEASURED, 3000 * (min(occ) + max(occ)), 3000 * (max(occ) - min(occ))
            else:
                src, hz, dev = FALLBACK, fb[s], 0
            idx = index_of(hz)
        o["n_counted"], o["source"], o["centre_hz"], o["deviation_hz"], o["index"] = cnt, src, hz, dev, idx
        out[e] = o
    return out, _next_centre_state(len(dec), out)


def auto_tracks(dec, mask_or_thresh, runs, smooth, head, fallback=None, state=None, base=None, max_samples=None, brute=False):
    """One submit of the auto-centre track: the centre records, then the track about every entry's own index.  state: (the
    track's, the centres') of the submit before, or None -> (centre records, track records, words, the state behind the submit)."""
    tst, cst = state if state is not None else (None, None)
    cen, cst = (head_centres_bruteforce if brute else head_centres)(dec, mask_or_thresh, runs, head, fallback, cst, base)
    recs, words, tst = (tracks_bruteforce if brute else tracks)(dec, mask_or_thresh, runs, smooth, None, tst, base, max_samples,
                                                                 run_index=cen["index"])
    return cen, recs, words, (tst, cst)


def merge_centres(pieces):
    """A chain's centre records (in order) -> the uncut run's: the first piece's, with the chain's flags (track.merge's) and the
    pieces' n_samples added.  The chain's first piece decides for the whole chain."""
    pieces = list(pieces)
    o = pieces[0].copy()
    for p in pieces[1:]:
        assert p["stream"] == o["stream"] and int(p["flags"]) & RUN_CONTINUES
        o["n_samples"] = int(o["n_samples"]) + int(p["n_samples"])
    o["flags"] = (int(pieces[0]["flags"]) & RUN_CONTINUES) | (int(pieces[-1]["flags"]) & RUN_OPEN)
    return o


def centre_chains(submits, restarts=None):
    """submits: one CENTRE_DTYPE array per submit, in order -> the merged records, in burst.chains' order."""
    return burst.chains(submits, restarts, join=merge_centres)


def centre_line(name: str, rec) -> str:
    """tfrec_gpu -G rate,auto: centre <file> <start_sample> <n_samples> <n_counted> <centre_hz> <deviation_hz|-> <m|f|i>, ahead of
    the burst's bits line; the deviation only of a measured centre; i: a chain whose first piece the output does not hold."""
    src = int(rec["source"])
    return "centre %s %d %d %d %d %s %s" % (name, int(rec["start_sample"]), int(rec["n_samples"]), int(rec["n_counted"]),
                                            int(rec["centre_hz"]), "%d" % int(rec["deviation_hz"]) if src == MEASURED else "-", "mfi"[src])


def bits_of(rec, words):
    """A record's track out of its submit's bitmap -> uint8 [n_samples]."""
    b0, n = int(rec["bit_offset"]), int(rec["n_samples"])
    w = np.asarray(words, dtype="<u4")[b0 // 32:(b0 + n + 31) // 32]
    return np.unpackbits(w.view(np.uint8), bitorder="little")[b0 % 32:b0 % 32 + n]


class Piece:
    """A record with its track; read like the record (burst.chains looks at stream and flags)."""

    def __init__(self, rec, bits):
        self.rec, self.bits = rec, np.asarray(bits, dtype=np.uint8)

    def __getitem__(self, f):
        return self.rec[f]

    def __setitem__(self, f, v):
        self.rec[f] = v


def merge(pieces):
    """A chain of pieces (in order; piece i + 1 has CONTINUES, piece i OPEN, one stream) -> one Piece, that of the uncut run: the
    tracks concatenated, n_samples and n_ones added, last_over the last piece's that has one, offset by the samples ahead of it;
    the first piece's stream, start_sample, thresh, bit_offset and CONTINUES, the last one's OPEN."""
    pieces = list(pieces)
    o = pieces[0].rec.copy()
    for p in pieces[1:]:
        assert p["stream"] == o["stream"] and int(p["flags"]) & RUN_CONTINUES
        if int(p["last_over"]) >= 0:
            o["last_over"] = int(o["n_samples"]) + int(p["last_over"])
        o["n_samples"] = int(o["n_samples"]) + int(p["n_samples"])
        o["n_ones"] = int(o["n_ones"]) + int(p["n_ones"])
    o["flags"] = (int(pieces[0]["flags"]) & RUN_CONTINUES) | (int(pieces[-1]["flags"]) & RUN_OPEN)
    return Piece(o, np.concatenate([p.bits for p in pieces]))


def chains(submits, restarts=None):
    """submits: one (records, words) per submit, in order -> the merged bursts as Pieces, in burst.chains' order (as they end; a
    chain still open behind the last submit last, by stream).  restarts: {submit index: streams that restart with it}."""
    return burst.chains([[Piece(r, bits_of(r, w)) for r in recs] for recs, w in submits], restarts, join=merge)


def sym(l: int, rate: int) -> int:
    return (2 * int(l) * int(rate) + 384000) // 768000


def slice_bits(bits, rate: int) -> list:
    """The header's Slicing: the maximal runs of equal value in order; a run too short for a symbol joins the run ahead of it
    (ahead of the first kept run it is dropped) -> the symbols, a list of 0 / 1."""
    b = np.asarray(bits, dtype=np.uint8)
    out = []
    if len(b) == 0:
        return out
    edges = np.flatnonzero(np.diff(b)) + 1
    starts = np.concatenate([[0], edges])
    lens = np.diff(np.concatenate([starts, [len(b)]]))
    kept = None  # (v, l)
    for w, m in zip(b[starts].tolist(), lens.tolist()):
        if kept is None:
            if sym(m, rate):
                kept = (w, m)
        elif sym(m, rate) == 0 or w == kept[0]:
            kept = (kept[0], kept[1] + m)
        else:
            out += [kept[0]] * sym(kept[1], rate)
            kept = (w, m)
    if kept is not None:
        out += [kept[0]] * sym(kept[1], rate)
    return out


def hex_of(symbols) -> str:
    """MSB-first, the last nibble zero-padded."""
    s = list(symbols) + [0] * (-len(symbols) % 4)
    return "".join("%x" % (8 * s[i] + 4 * s[i + 1] + 2 * s[i + 2] + s[i + 3]) for i in range(0, len(s), 4))


def line(name: str, piece, rate: int) -> str:
    """tfrec_gpu -G: bits <file> <start_sample> <n_samples> <burst_samples> <n_bits>[+] <hex|->: the slice of the track's first
    burst_samples = last_over + 1 samples, of the first 2^20 at most (then the + behind n_bits: n_samples > 2^20)."""
    rec = piece.rec
    length = int(rec["last_over"]) + 1
    symbols = slice_bits(piece.bits[:KEEP][:length], rate)
    return "bits %s %d %d %d %d%s %s" % (name, int(rec["start_sample"]), int(rec["n_samples"]), length, len(symbols),
                                         "+" if int(rec["n_samples"]) > KEEP else "", hex_of(symbols) if symbols else "-")


def smooth_of(rate: int) -> int:
    """tfrec_gpu -G's L: half a symbol, (384000 + rate) // (2 rate) held within 1 .. 16."""
    return max(1, min(AHEAD, (384000 + int(rate)) // (2 * int(rate))))


def device_bytes(n_streams: int, max_runs: int, max_samples: int) -> int:
    """What tfrec_amd_enable_burst_track adds to tfrec_amd_get_memory's device bytes: per FIFO set the records, the bitmap and the
    centre indices; per stream the carried 16 pairs and prior."""
    from .api import FIFO_DEPTH
    return FIFO_DEPTH * (max_runs * TRACK_DTYPE.itemsize + 4 * ((max_samples + 31) // 32) + 4 * n_streams) + n_streams * (4 * AHEAD + 4)


def pinned_bytes(n_streams: int) -> int:
    """... and to its page-locked bytes: the centre indices' source per FIFO set."""
    from .api import FIFO_DEPTH
    return FIFO_DEPTH * 4 * n_streams


def auto_device_bytes(n_streams: int, max_runs: int, max_samples: int) -> int:
    """What tfrec_amd_enable_burst_track_auto adds to the device bytes: the track's, per FIFO set the centre records, per stream the
    carried index and centre."""
    from .api import FIFO_DEPTH
    return device_bytes(n_streams, max_runs, max_samples) + FIFO_DEPTH * max_runs * CENTRE_DTYPE.itemsize + 8 * n_streams


# ---- the phase track (tfrec_amd_enable_burst_track_phase, the header's "Phase track")
PHASE_AHEAD = 80  # the pairs carried from submit to submit: LAG_MAX + AHEAD, what c(k) >= m and z[k - i - m] can reach back to
LAG_MIN, LAG_MAX = 1, 64  # m


def lag_of(rate: int) -> int:
    """tfrec_gpu -G rate,psk's m: a symbol in samples, floor((768000 + rate) / (2 rate)) (a usage error above 64)."""
    return (768000 + int(rate)) // (2 * int(rate))


def fresh_phase_state(n_streams: int) -> dict:
    """What a phase context carries before its first submit: no pairs, no chain."""
    return {"carry": np.zeros((n_streams, PHASE_AHEAD, 2), dtype=np.int16), "prior": np.zeros(n_streams, dtype=np.int64)}


def _next_phase_state(dec, runs, state):
    """The state behind the submit: every stream's last 80 pairs, and prior = min(80, prior' + n) of the stream's OPEN run."""
    nxt = {"carry": np.array([burst._pairs(d)[-PHASE_AHEAD:] for d in dec], dtype=np.int16), "prior": np.zeros(len(dec), dtype=np.int64)}
    for r in runs:
        if int(r["flags"]) & RUN_OPEN:
            s = int(r["stream"])
            before = int(state["prior"][s]) if int(r["flags"]) & RUN_CONTINUES else 0
            nxt["prior"][s] = min(PHASE_AHEAD, before + int(r["n_samples"]))
    return nxt


def carrier_index(A: int, B: int) -> int:
    """The header's search, vectorised: the smallest r of 0 .. 4095 with score(r) = A C[r] + B S[r] > 0 that minimises
    |cross(r)| = |B C[r] - A S[r]|; |A|, |B| < 2^43, so both stay below 2^59.  (A, B) != (0, 0)."""
    A, B = int(A), int(B)
    assert (A or B) and abs(A) < 1 << 43 and abs(B) < 1 << 43
    c, s_ = tune.table()
    c, s_ = c.astype(np.int64), s_.astype(np.int64)
    score, cross = A * c + B * s_, np.abs(B * c - A * s_)
    return int(np.argmin(np.where(score > 0, cross, np.iinfo(np.int64).max)))  # (argmin: the first of equal minima)


def carrier_index_bruteforce(A: int, B: int) -> int:
    """The same over all 4096 candidates in Python integers."""
    c, s_ = tune.table()
    best = None
    for r in range(4096):
        C, S = int(c[r]), int(s_[r])
        if A * C + B * S > 0 and (best is None or abs(B * C - A * S) < best[0]):
            best = (abs(B * C - A * S), r)
    return best[1]


def carrier_hz(r: int) -> int:
    """centre_hz of a measured index: floor(375 rs / 4), rs = r below 2048 and r - 4096 otherwise."""
    return 375 * (r if r < 2048 else r - 4096) // 4


def head_carriers(dec, mask_or_thresh, runs, head, fallback=None, state=None, base=None):
    """One submit's carrier records: head_centres' arguments, results and carried state, the centre of an entry without
    CONTINUES measured as the header's "Phase track" words it -- the sums A, B of the head's counted products and the zero of the
    cross term over the 4096 table directions."""
    K = int(head)
    assert HEAD_MIN <= K <= HEAD_MAX
    state = fresh_centre_state(len(dec)) if state is None else state
    fb = _fallbacks(fallback, len(dec))
    out = np.zeros(len(runs), dtype=CENTRE_DTYPE)
    rows = _Rows(dec, mask_or_thresh)
    for e, r in enumerate(runs):
        s, a, n, cont = _window(dec, r, base)
        o = _centre_copied(r)
        if cont:
            if int(state["index"][s]) >= 0:
                o["source"], o["centre_hz"], o["index"] = INHERITED, int(state["centre_hz"][s]), int(state["index"][s])
            else:
                o["source"], o["centre_hz"], o["index"] = FALLBACK, fb[s], index_of(fb[s])
            out[e] = o
            continue
        nh = min(n, K)
        over = rows.over(s)[a:a + nh]
        z = rows.pairs(s)[a:a + nh]
        I, Q, Ip, Qp = z[1:, 0], z[1:, 1], z[:-1, 0], z[:-1, 1]
        both = over[1:] & over[:-1]
        A, B = int((I * Ip + Q * Qp)[both].sum()), int((Q * Ip - I * Qp)[both].sum())
        P = int(np.count_nonzero(both))
        o["n_counted"] = P
        if P >= COUNT_MIN and (A or B):
            ri = carrier_index(A, B)
            o["source"], o["centre_hz"], o["index"] = MEASURED, carrier_hz(ri), ri
        else:
            o["source"], o["centre_hz"], o["index"] = FALLBACK, fb[s], index_of(fb[s])
        out[e] = o
    return out, _next_centre_state(len(dec), out)


def head_carriers_bruteforce(dec, mask_or_thresh, runs, head, fallback=None, state=None, base=None):
    """The same, one sample and one candidate at a time in Python integers, as the header words it."""
    K = int(head)
    state = fresh_centre_state(len(dec)) if state is None else state
    fb = _fallbacks(fallback, len(dec))
    out = np.zeros(len(runs), dtype=CENTRE_DTYPE)
    for e, r in enumerate(runs):
        s, a, n, cont = _window(dec, r, base)
        o = _centre_copied(r)
        cnt = 0
        if cont:
            idx = int(state["index"][s])
            src, hz = (INHERITED, int(state["centre_hz"][s])) if idx >= 0 else (FALLBACK, fb[s])
            idx = idx if idx >= 0 else index_of(hz)
        else:
            row = burst._pairs(dec[s]).tolist()
            over = envelope._over(burst._pairs(dec[s]).astype(np.int64), mask_or_thresh[s]).tolist()
            A = B = 0
            for k in range(1, min(n, K)):
                if over[a + k] and over[a + k - 1]:
                    (i, q), (ip, qp) = row[a + k], row[a + k - 1]
                    A, B, cnt = A + i * ip + q * qp, B + q * ip - i * qp, cnt + 1
            if cnt >= COUNT_MIN and (A or B):
                idx = carrier_index_bruteforce(A, B)
                src, hz = MEASURED, carrier_hz(idx)
            else:
                src, hz = FALLBACK, fb[s]
                idx = index_of(hz)
        o["n_counted"], o["source"], o["centre_hz"], o["index"] = cnt, src, hz, idx
        out[e] = o
    return out, _next_centre_state(len(dec), out)


def _phase_settings(smooth, lag):
    L, m = int(smooth), int(lag)
    assert 1 <= L <= AHEAD and LAG_MIN <= m <= LAG_MAX
    return L, m


def phase_tracks(dec, mask_or_thresh, runs, smooth, lag, head, fallback=None, state=None, base=None, max_samples=None):
    """One submit of the phase track: the carrier records (head_carriers), then per entry the differential detector at lag m
    about the entry's index r: u[k] = dm C[rm] + cm S[rm], rm = r m mod 4096, of the pairs at k and k - m, 0 where the chain holds
    fewer than m samples ahead of k; t[k] = 1 iff the sum of u[k - i] over i < L is greater than 0.  state: (the 80 pairs and prior,
    the centres') of the submit before, or None -> (carrier records, track records, words, the state behind the submit)."""
    L, m = _phase_settings(smooth, lag)
    pst, cst = state if state is not None else (None, None)
    pst = fresh_phase_state(len(dec)) if pst is None else pst
    cen, cst = head_carriers(dec, mask_or_thresh, runs, head, fallback, cst, base)
    c, s_ = tune.table()
    out = np.zeros(len(runs), dtype=TRACK_DTYPE)
    tr = []
    H = PHASE_AHEAD
    rows = _Rows(dec, mask_or_thresh, pst["carry"])
    for e, r in enumerate(runs):
        s, a, n, cont = _window(dec, r, base)
        rm = int(cen[e]["index"]) * m % 4096
        C, S = int(c[rm]), int(s_[rm])
        z = rows.extended(s)
        cf = a - (int(pst["prior"][s]) if cont else 0)  # the chain's first sample, submit-relative (>= -80)
        k = np.arange(a - (AHEAD - 1), a + n)  # every sample a product may be needed of; z's index is k + 80
        ok = k - cf >= m  # (then k - m >= cf >= -80)
        kk = np.where(ok, k, m)  # (a harmless index where the product is not used)
        I, Q, Ip, Qp = z[kk + H, 0], z[kk + H, 1], z[kk + H - m, 0], z[kk + H - m, 1]
        u = np.where(ok, (I * Ip + Q * Qp) * C + (Q * Ip - I * Qp) * S, 0)  # (|u| < 2^47)
        cs = np.concatenate([[0], np.cumsum(u)])
        p = np.arange(n) + AHEAD  # sample a + j is u[j + 15]: the sum of u[j + 16 - L .. j + 15]
        t = (cs[p] - cs[p - L]) > 0
        o = _copied(r)
        over = rows.over(s)[a:a + n]
        idx = np.flatnonzero(over)
        o["last_over"] = int(idx[-1]) if len(idx) else -1
        o["n_ones"] = int(np.count_nonzero(t))
        out[e] = o
        tr.append(t.astype(np.uint8))
    return cen, out, _pack(out, tr, max_samples), (_next_phase_state(dec, runs, pst), cst)


def phase_tracks_bruteforce(dec, mask_or_thresh, runs, smooth, lag, head, fallback=None, state=None, base=None, max_samples=None):
    """The same, one sample at a time in Python integers, as the header words it: c(k) counts from the chain's first sample."""
    L, m = _phase_settings(smooth, lag)
    pst, cst = state if state is not None else (None, None)
    pst = fresh_phase_state(len(dec)) if pst is None else pst
    cen, cst = head_carriers_bruteforce(dec, mask_or_thresh, runs, head, fallback, cst, base)
    c, s_ = tune.table()
    out = np.zeros(len(runs), dtype=TRACK_DTYPE)
    tr = []
    for e, r in enumerate(runs):
        s, a, n, cont = _window(dec, r, base)
        rm = int(cen[e]["index"]) * m % 4096
        C, S = int(c[rm]), int(s_[rm])
        row = burst._pairs(dec[s]).tolist()
        ahead = np.asarray(pst["carry"][s]).reshape(PHASE_AHEAD, 2).tolist()
        prior = int(pst["prior"][s]) if cont else 0
        over = envelope._over(burst._pairs(dec[s]).astype(np.int64), mask_or_thresh[s]).tolist()

        def z(k):  # run-relative; k < 0 only in a CONTINUES run, whose a == 0
            return row[a + k] if a + k >= 0 else ahead[PHASE_AHEAD + a + k]

        def u(k):
            if k + prior < m:  # c(k) < m (c(k) < 0: ahead of the chain)
                return 0
            (i, q), (ip, qp) = z(k), z(k - m)
            return (i * ip + q * qp) * C + (q * ip - i * qp) * S

        t, last = [], -1
        for k in range(n):
            total = 0
            for i in range(L):
                total += u(k - i)
            t.append(1 if total > 0 else 0)
            if over[a + k]:
                last = k
        o = _copied(r)
        o["last_over"], o["n_ones"] = last, sum(t)
        out[e] = o
        tr.append(np.array(t, dtype=np.uint8))
    return cen, out, _pack(out, tr, max_samples), (_next_phase_state(dec, runs, pst), cst)


def phase_device_bytes(n_streams: int, max_runs: int, max_samples: int) -> int:
    """What tfrec_amd_enable_burst_track_phase adds to the device bytes: per FIFO set the track records, the bitmap, the set centres
    and the centre records; per stream the carried 80 pairs, prior and the carried index and centre."""
    from .api import FIFO_DEPTH
    return (FIFO_DEPTH * (max_runs * (TRACK_DTYPE.itemsize + CENTRE_DTYPE.itemsize) + 4 * ((max_samples + 31) // 32) + 4 * n_streams) +
            n_streams * (4 * PHASE_AHEAD + 4 + 8))
