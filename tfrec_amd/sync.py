"""The burst sync (tfrec_amd_enable_burst_sync, include/tfrec_amd.h: tfrec_amd_burst_sync) restated in numpy -- no GPU
needed.  Written from the header's definition alone; exact integers throughout.

Per captured sample of every run of the recorder's table one bit: 1 where the burst track, sampled at P symbol centres that end
at the sample, differs from a sync word in at most E places (under BOTH: or agrees in at most E) -- packed where the track's bit
lies; per run a 48-byte record.  The framing turns a merged track and match track into the frames behind each sync word.  Nothing
here has been measured on real recordings.

  Settings           rate, pattern, P, E and BOTH, checked as the enable call checks them;
  deltas             delta(0 .. n - 1);
  syncs              vectorised, from the definition: one submit's records and match bitmap from the submit's track records and
                     track bitmap and the state the submit before left;
  syncs_bruteforce   the same sample by sample, in Python integers;
  bits_of            a record's match track out of the bitmap;  merge: a chain of pieces -> the record and match track of the
                     uncut run;  chains: the chains of a sequence of submits (burst.chains' walk);
  frames             a merged track and match track -> the frames;  line: tfrec_gpu -Y's output line (lsb: the byte order);
  device_bytes       what tfrec_amd_enable_burst_sync adds to tfrec_amd_get_memory (pinned_bytes: nothing).
"""
from __future__ import annotations

import numpy as np

from . import burst, track
from .capture import RUN_CONTINUES, RUN_OPEN

HISTORY = 2047  # the track bits carried from submit to submit, and the largest span
NONE = 0xFFFFFFFF  # best where no d is defined
BOTH = 1  # the flag: the complemented pattern matches too
KEEP = track.KEEP  # the samples of a chain's tracks the host keeps
SYNC_DTYPE = np.dtype([("stream", "<u4"), ("flags", "<u4"), ("start_sample", "<i8"), ("n_samples", "<u4"), ("thresh", "<i4"),
                       ("bit_offset", "<u8"), ("n_hits", "<u4"), ("best", "<u4"), ("best_at", "<u4"), ("reserved", "<u4")])
assert SYNC_DTYPE.itemsize == 48


def deltas(rate: int, n: int) -> list:
    """delta(i) = floor((768000 i + R) / (2 R)) for i = 0 .. n - 1: the samples from a symbol's centre to the centre i symbols on."""
    R = int(rate)
    return [(768000 * i + R) // (2 * R) for i in range(int(n))]


class Settings:
    """What tfrec_amd_enable_burst_sync fixes; a ValueError where it returns E_INVAL."""

    def __init__(self, rate: int, pattern: int, n_bits: int, max_errors: int = 0, both: bool = False):
        self.rate, self.P, self.E, self.both = int(rate), int(n_bits), int(max_errors), bool(both)
        if not 1000 <= self.rate <= 96000:
            raise ValueError("rate %d outside 1000 .. 96000" % self.rate)
        if not 8 <= self.P <= 64:
            raise ValueError("%d pattern bits outside 8 .. 64" % self.P)
        if self.E < 0 or 2 * self.E >= self.P:
            raise ValueError("%d errors outside 0 <= E < P / 2" % self.E)
        self.pattern = int(pattern) & ((1 << self.P) - 1)
        self.delta = deltas(self.rate, self.P)
        self.span = self.delta[-1]
        if self.span > HISTORY:
            raise ValueError("span %d above %d" % (self.span, HISTORY))
        self.bit = [(self.pattern >> j) & 1 for j in range(self.P)]  # bit 0: the last one transmitted

    @property
    def flags(self) -> int:
        return BOTH if self.both else 0

    def hit(self, d: int) -> bool:
        return d <= self.E or (self.both and d >= self.P - self.E)

    def folded(self, d: int) -> int:
        return min(d, self.P - d) if self.both else d


def fresh_state(n_streams: int) -> dict:
    """What a context carries before its first submit: no history."""
    return {"bits": [np.zeros(0, dtype=np.uint8) for _ in range(n_streams)]}


def _fits(rec, max_samples) -> bool:
    return max_samples is None or int(rec["bit_offset"]) + int(rec["n_samples"]) <= max_samples


def _copied(rec):
    o = np.zeros((), dtype=SYNC_DTYPE)
    for f in ("stream", "flags", "start_sample", "n_samples", "thresh", "bit_offset"):
        o[f] = rec[f]
    o["best"] = NONE
    return o


def _history(rec, state):
    h = state["bits"][int(rec["stream"])] if int(rec["flags"]) & RUN_CONTINUES else np.zeros(0, dtype=np.uint8)
    return np.asarray(h, dtype=np.uint8)[-HISTORY:]


def _next_state(n_streams, trecs, tr, state, max_samples):
    """The state behind the submit: per stream the last 2047 bits of the chain its OPEN run belongs to, as far as they were
    available to it; nothing behind a run that does not fit max_samples, and nothing without an OPEN run."""
    nxt = fresh_state(n_streams)
    for r, t in zip(trecs, tr):
        if int(r["flags"]) & RUN_OPEN and _fits(r, max_samples):
            nxt["bits"][int(r["stream"])] = np.concatenate([_history(r, state), t])[-HISTORY:]
    return nxt


def _tracks(trecs, twords, max_samples):
    return [track.bits_of(r, twords) if _fits(r, max_samples) else np.zeros(int(r["n_samples"]), dtype=np.uint8) for r in trecs]


def syncs(trecs, twords, settings: Settings, state=None, n_streams=None, max_samples=None):
    """One submit.  trecs, twords: the submit's track records and track bitmap (read_burst_tracks'; the records carry the table
    entry and its place in the pool); state: what the submit before returned (default: a fresh context's); n_streams: the
    context's (default: as many as the state or the records name); max_samples: the pool's size (default: everything fits) ->
    (a SYNC_DTYPE array, one record per track record; the match bitmap's uint32 words, as many as the pairs that fit need; the state behind
    the submit)."""
    st = settings
    if n_streams is None:
        n_streams = len(state["bits"]) if state is not None else int(max([int(r["stream"]) for r in trecs], default=-1)) + 1
    state = fresh_state(n_streams) if state is None else state
    tr = _tracks(trecs, twords, max_samples)
    out = np.zeros(len(trecs), dtype=SYNC_DTYPE)
    ms = []
    for e, (r, t) in enumerate(zip(trecs, tr)):
        o = _copied(r)
        n = len(t)
        m = np.zeros(n, dtype=np.uint8)
        if _fits(r, max_samples):
            h = _history(r, state)
            H = len(h)
            ext = np.concatenate([h, t]).astype(np.int64)
            k0 = max(0, st.span - H)  # the first defined k
            if k0 < n:
                d = np.zeros(n - k0, dtype=np.int64)
                for j in range(st.P):
                    a = H + k0 - st.delta[j]
                    d += ext[a:a + n - k0] != st.bit[j]
                hit = d <= st.E
                if st.both:
                    hit |= d >= st.P - st.E
                m[k0:] = hit
                f = np.minimum(d, st.P - d) if st.both else d
                at = int(np.argmin(f))  # (the first minimum)
                o["n_hits"], o["best"], o["best_at"] = int(np.count_nonzero(hit)), int(f[at]), k0 + at
        out[e] = o
        ms.append(m)
    return out, track._pack(out, ms, max_samples), _next_state(n_streams, trecs, tr, state, max_samples)


def syncs_bruteforce(trecs, twords, settings: Settings, state=None, n_streams=None, max_samples=None):
    """The same, one sample at a time in Python integers, as the header words it: d[k] counts the j with t[k - delta(j)] != bit j."""
    st = settings
    if n_streams is None:
        n_streams = len(state["bits"]) if state is not None else int(max([int(r["stream"]) for r in trecs], default=-1)) + 1
    state = fresh_state(n_streams) if state is None else state
    tr = _tracks(trecs, twords, max_samples)
    out = np.zeros(len(trecs), dtype=SYNC_DTYPE)
    ms = []
    for e, (r, t) in enumerate(zip(trecs, tr)):
        o = _copied(r)
        tl = t.tolist()
        m = [0] * len(tl)
        if _fits(r, max_samples):
            h = _history(r, state).tolist()
            H = len(h)

            def bit(k):  # t[k], k >= -H
                return tl[k] if k >= 0 else h[H + k]

            hits, best, best_at = 0, NONE, 0
            for k in range(len(tl)):
                if k + H < st.span:
                    continue
                d = sum(1 for j in range(st.P) if bit(k - st.delta[j]) != st.bit[j])
                if st.hit(d):
                    m[k] = 1
                    hits += 1
                if st.folded(d) < best:
                    best, best_at = st.folded(d), k
            o["n_hits"], o["best"], o["best_at"] = hits, best, best_at
        out[e] = o
        ms.append(np.array(m, dtype=np.uint8))
    return out, track._pack(out, ms, max_samples), _next_state(n_streams, trecs, tr, state, max_samples)


bits_of = track.bits_of  # a record's match track out of its submit's bitmap -> uint8 [n_samples]


class Piece(track.Piece):
    """A sync record with its match track."""


def merge(pieces):
    """A chain of pieces (in order, as for track.merge) -> one Piece, that of the uncut run: the match tracks concatenated,
    n_samples and n_hits added, the smaller best -- on a tie the earlier piece's -- with its best_at offset by the samples ahead;
    the flags as track.merge's."""
    pieces = list(pieces)
    o = pieces[0].rec.copy()
    for p in pieces[1:]:
        assert p["stream"] == o["stream"] and int(p["flags"]) & RUN_CONTINUES
        if int(p["best"]) < int(o["best"]):
            o["best"], o["best_at"] = int(p["best"]), int(o["n_samples"]) + int(p["best_at"])
        o["n_samples"] = int(o["n_samples"]) + int(p["n_samples"])
        o["n_hits"] = int(o["n_hits"]) + int(p["n_hits"])
    o["flags"] = (int(pieces[0]["flags"]) & RUN_CONTINUES) | (int(pieces[-1]["flags"]) & RUN_OPEN)
    return Piece(o, np.concatenate([p.bits for p in pieces]))


def chains(submits, restarts=None):
    """submits: one (records, words) per submit, in order -> the merged bursts as Pieces, in track.chains' order."""
    return burst.chains([[Piece(r, bits_of(r, w)) for r in recs] for recs, w in submits], restarts, join=merge)


def plateaus(m) -> list:
    """The maximal runs [a, b] of ones in m."""
    x = np.concatenate([[0], np.asarray(m, dtype=np.int8), [0]])
    e = np.flatnonzero(np.diff(x))
    return [(int(a), int(b) - 1) for a, b in zip(e[0::2], e[1::2])]


class LsbBits(list):
    """A payload's bits, in the order received, that line() prints LSB-first per byte."""


def hex_of(bits, lsb: bool = False) -> str:
    """The payload's hex: MSB-first with the last nibble zero-padded (track.hex_of) -- or, lsb, every byte assembled with the first
    received bit as bit 0, a last partial byte zero-filled at the top, always two digits a byte."""
    if not lsb:
        return track.hex_of(bits)
    b = list(bits)
    return "".join("%02x" % sum(v << i for i, v in enumerate(b[k:k + 8])) for k in range(0, len(b), 8))


def frames(tpiece, spiece, settings: Settings, n_bytes: int = 8, lsb: bool = False) -> list:
    """The header's Framing on a chain's merged track (a track.Piece) and match track (a Piece) -> [(c, errors, '+' or '-', the
    payload's bits as a list)], in the order of c.  lsb: the list is an LsbBits, which line() prints LSB-first per byte; the bits
    and their number are the same."""
    st = settings
    length = min(int(tpiece.rec["last_over"]) + 1, KEEP, len(tpiece.bits))
    t = tpiece.bits[:length].tolist()
    out = []
    for a, b in plateaus(spiece.bits[:length]):
        c = (a + b) >> 1
        d = sum(1 for j in range(st.P) if (t[c - st.delta[j]] if c >= st.delta[j] else 0) != st.bit[j])  # (ahead of the track: 0)
        plus = d <= st.E
        pay = []
        for i in range(1, 8 * int(n_bytes) + 1):
            q = c + (768000 * i + st.rate) // (2 * st.rate)
            if q >= length:
                break
            pay.append(t[q] if plus else 1 - t[q])
        out.append((c, d if plus else st.P - d, "+" if plus else "-", LsbBits(pay) if lsb else pay))
    return out


def line(name: str, spiece, frame, lsb: bool = False) -> str:
    """tfrec_gpu -Y: frame <file> <start_sample> <sync_sample> <errors> <+|-> <n_bits> <hex|->; lsb (or a frame of frames(...,
    lsb=True)): the hex LSB-first per byte."""
    c, errors, pol, pay = frame
    start = int(spiece.rec["start_sample"])
    lsb = lsb or isinstance(pay, LsbBits)
    return "frame %s %d %d %d %s %d %s" % (name, start, start + c, errors, pol, len(pay), hex_of(pay, lsb) if pay else "-")


def device_bytes(n_streams: int, max_runs: int, max_samples: int) -> int:
    """What tfrec_amd_enable_burst_sync adds to tfrec_amd_get_memory's device bytes: per FIFO set the records and the match
    bitmap; per stream the carried 64 words and H."""
    from .api import FIFO_DEPTH
    return FIFO_DEPTH * (max_runs * SYNC_DTYPE.itemsize + 4 * ((max_samples + 31) // 32)) + n_streams * (4 * 64 + 4)


def pinned_bytes(n_streams: int) -> int:
    """... and to its page-locked bytes: nothing."""
    return 0
