"""The pulse slicer (tfrec_amd_enable_burst_symbols, include/tfrec_amd.h: "Pulse slicer") restated in Python integers
-- no GPU needed.  Written from the header's definition alone; exact integers throughout.

An optional stage of the burst track for pulse-width and pulse-gap keyed bursts: per run of the recorder's table a stream of symbols
-- short, long or break, one per deciding edge by the length of the stretch of equal track bits ahead of it --, as two bitmaps
(value, break mark) with symbol i of a run at bit bit_offset + i, and a 48-byte record.  Nothing here has been measured on real
recordings.

  Settings           mode, lo, mid, hi and SHORT_ONE, checked as the enable call checks them;
  symbols_bruteforce one submit's records and two bitmaps from the submit's track records and track bitmap and the state the submit
                     before left, sample by sample as the header words it;
  merge, chains      the chains of a sequence of submits: the symbol streams concatenated, the counts added;
  text, line         tfrec_gpu -J's symbols line;
  device_bytes       what tfrec_amd_enable_burst_symbols adds to tfrec_amd_get_memory (pinned_bytes: nothing).
"""
from __future__ import annotations

import numpy as np

from . import burst, track
from .capture import RUN_CONTINUES, RUN_OPEN
from .linecode import HISTORY, _begin, _fits, _history, _next_state, _tracks, fresh_state  # the line code's history rule  # noqa: F401

WIDTH, GAP = 0, 1  # the modes
SHORT_ONE = 1  # the flag: a short stretch reads 1
CAP = 2047  # a stretch is counted this far
LISTED = 2048  # the symbols tfrec_gpu -J lists
SYMBOLS_DTYPE = np.dtype([("stream", "<u4"), ("flags", "<u4"), ("start_sample", "<i8"), ("n_samples", "<u4"), ("thresh", "<i4"),
                          ("bit_offset", "<u8"), ("n_symbols", "<u4"), ("n_breaks", "<u4"), ("n_glitches", "<u4"), ("reserved", "<u4")])
assert SYMBOLS_DTYPE.itemsize == 48


class Settings:
    """What tfrec_amd_enable_burst_symbols fixes; a ValueError where it returns E_INVAL."""

    def __init__(self, mode: int, lo: int, mid: int, hi: int, short_one: bool = False):
        self.mode, self.lo, self.mid, self.hi, self.short_one = int(mode), int(lo), int(mid), int(hi), bool(short_one)
        if self.mode not in (WIDTH, GAP):
            raise ValueError("mode %d: WIDTH or GAP" % self.mode)
        if not 1 <= self.lo <= self.mid <= self.hi <= CAP - 1:
            raise ValueError("want 1 <= lo <= mid <= hi <= 2046, got %d, %d, %d" % (self.lo, self.mid, self.hi))

    @property
    def flags(self) -> int:
        return SHORT_ONE if self.short_one else 0


def decide(t, h, st: Settings):
    """One piece: its track t[0 .. n) and the H available bits h ahead of it -> (the symbols in order of k, each 0, 1 or "/" for a
    break; the glitches)."""
    H, out, glitches = len(h), [], 0

    def bit(x):  # t[x]
        return t[x] if x >= 0 else h[H + x] if x >= -H else 0

    for k in range(len(t)):
        prev = bit(k - 1)
        if (t[k], prev) != ((0, 1) if st.mode == WIDTH else (1, 0)):
            continue  # no deciding edge
        l = 0  # l(k): the consecutive x = k - 1, k - 2, ... >= -H with t[x] = t[k - 1], counted to 2047
        while l < CAP and k - 1 - l >= -H and bit(k - 1 - l) == prev:
            l += 1
        if st.mode == GAP and l == k + H < CAP:  # the stretch reaches the chain's start
            out.append("/")
        elif l < st.lo:
            glitches += 1
        elif l < st.mid:
            out.append(1 if st.short_one else 0)
        elif l <= st.hi:
            out.append(0 if st.short_one else 1)
        else:
            out.append("/")
    return out, glitches


def symbols_bruteforce(trecs, twords, settings: Settings, state=None, n_streams=None, max_samples=None):
    """One submit.  trecs, twords: the submit's track records and track bitmap (read_burst_tracks'); state: what the submit before
    returned (default: a fresh context's); max_samples: the pool's size (default: everything fits) -> (a SYMBOLS_DTYPE array, one
    record per track record; the bits bitmap's and the marks bitmap's uint32 words, as many as the pairs that fit need; the state
    behind the submit)."""
    n_streams, state = _begin(trecs, state, n_streams)
    tr = _tracks(trecs, twords, max_samples)
    out = np.zeros(len(trecs), dtype=SYMBOLS_DTYPE)
    vals, marks = [], []
    for e, (r, t) in enumerate(zip(trecs, tr)):
        for f in ("stream", "flags", "start_sample", "n_samples", "thresh", "bit_offset"):
            out[e][f] = r[f]
        sy, gl = decide(t.tolist(), _history(r, state).tolist(), settings) if _fits(r, max_samples) else ([], 0)
        out[e]["n_symbols"], out[e]["n_breaks"], out[e]["n_glitches"] = len(sy), sy.count("/"), gl
        pad = [0] * (len(t) - len(sy))  # (at most (n + 1) / 2 symbols: inside the run's own bits)
        vals.append(np.array([int(x == 1) for x in sy] + pad, dtype=np.uint8))
        marks.append(np.array([int(x == "/") for x in sy] + pad, dtype=np.uint8))
    return out, track._pack(out, vals, max_samples), track._pack(out, marks, max_samples), _next_state(n_streams, trecs, tr, state, max_samples)


class Piece(track.Piece):
    """A record with its symbols' values (bits) and break marks, n_symbols of each."""

    def __init__(self, rec, bits, marks):
        track.Piece.__init__(self, rec, bits)
        self.marks = np.asarray(marks, dtype=np.uint8)


def piece_of(rec, bits, marks):
    one = dict(bit_offset=rec["bit_offset"], n_samples=rec["n_symbols"])
    return Piece(rec, track.bits_of(one, bits), track.bits_of(one, marks))


def merge(pieces):
    """A chain of pieces -> one Piece, that of the uncut run: the symbol streams concatenated, n_samples and the three counts added;
    the first piece's stream, start_sample, thresh, bit_offset and CONTINUES, the last one's OPEN."""
    pieces = list(pieces)
    o = pieces[0].rec.copy()
    for p in pieces[1:]:
        assert p["stream"] == o["stream"] and int(p["flags"]) & RUN_CONTINUES
        for f in ("n_samples", "n_symbols", "n_breaks", "n_glitches"):
            o[f] = int(o[f]) + int(p[f])
    o["flags"] = (int(pieces[0]["flags"]) & RUN_CONTINUES) | (int(pieces[-1]["flags"]) & RUN_OPEN)
    return Piece(o, np.concatenate([p.bits for p in pieces]), np.concatenate([p.marks for p in pieces]))


def chains(submits, restarts=None):
    """submits: one (records, bits words, marks words) per submit, in order -> the merged bursts as Pieces, in burst.chains' order."""
    return burst.chains([[piece_of(r, b, m) for r in recs] for recs, b, m in submits], restarts, join=merge)


def text(piece) -> str:
    """The first 2048 symbols as 0, 1 and / (a break)."""
    return "".join("/" if m else "%d" % v for v, m in zip(piece.bits[:LISTED].tolist(), piece.marks[:LISTED].tolist()))


def line(name: str, piece) -> str:
    """tfrec_gpu -J: symbols <file> <start_sample> <n_samples> <n_symbols>[+] <n_breaks> <n_glitches> <text|->; a + behind n_symbols
    marks more than the 2048 listed."""
    rec = piece.rec
    n = int(rec["n_symbols"])
    return "symbols %s %d %d %d%s %d %d %s" % (name, int(rec["start_sample"]), int(rec["n_samples"]), n, "+" if n > LISTED else "",
                                               int(rec["n_breaks"]), int(rec["n_glitches"]), text(piece) or "-")


def device_bytes(n_streams: int, max_runs: int, max_samples: int) -> int:
    """What tfrec_amd_enable_burst_symbols adds to tfrec_amd_get_memory's device bytes: per FIFO set the records and five bitmaps;
    per stream the carried 64 words and H."""
    from .api import FIFO_DEPTH
    return FIFO_DEPTH * (max_runs * SYMBOLS_DTYPE.itemsize + 5 * 4 * ((max_samples + 31) // 32)) + n_streams * (4 * 64 + 4)


def pinned_bytes(n_streams: int) -> int:
    """... and to its page-locked bytes: nothing."""
    return 0
