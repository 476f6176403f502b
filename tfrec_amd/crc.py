"""The frame check (tfrec_amd_enable_burst_crc, include/tfrec_amd.h: "Frame check") restated in numpy -- no GPU needed.
Written from the header's definition alone; exact integers throughout.

An optional stage of the burst track: per captured sample of every run of the recorder's table one bit, 1 where the N bytes whose
last bit sits at the sample -- read from the sync's input track at the Framing's symbol centres -- carry their own CRC, packed where
the track's bit lies; per run a 40-byte record.  The verdict of a frame that sync.frames found is then one bit of the merged check
track.  Nothing here has been measured on real recordings.

  Settings           rate, N, skip, width, poly, init, xorout, LSB and INVERT, checked as the enable call checks them; D; table()
                     and r0: the affine form, residue = r0 ^ XOR of col_i over the set bits at k - off_i;
  crcs               vectorised over the residue's planes, from the table: one submit's records and check bitmap from the
                     submit's input records and bitmap (the track's, or the line code's) and the state the submit before left;
  crcs_bruteforce    the same sample by sample, assembling bytes and running the bitwise CRC in Python integers;
  bits_of            a record's check track out of the bitmap;  merge: a chain of pieces -> the record and check track of the
                     uncut run;  chains: the chains of a sequence of submits (burst.chains' walk);
  verdicts           sync.frames' frames and the merged check track -> 'ok', 'bad' or '-' per frame;
  line               tfrec_gpu -V's line per burst;
  device_bytes       what tfrec_amd_enable_burst_crc adds to tfrec_amd_get_memory (pinned_bytes: nothing).
"""
from __future__ import annotations

import numpy as np

from . import burst, track
from .capture import RUN_CONTINUES, RUN_OPEN

HISTORY = 16383  # the input bits carried from submit to submit, and the largest D
NONE = 0xFFFFFFFF  # first_at where no sample checks
LSB = 1  # the flag: a byte's first received bit is its bit 0
INVERT = 2  # the flag: every bit is complemented before use
CRC_DTYPE = np.dtype([("stream", "<u4"), ("flags", "<u4"), ("start_sample", "<i8"), ("n_samples", "<u4"), ("thresh", "<i4"),
                      ("bit_offset", "<u8"), ("n_ok", "<u4"), ("first_at", "<u4")])
assert CRC_DTYPE.itemsize == 40


def delta(rate: int, i: int) -> int:
    """delta(i) = floor((768000 i + R) / (2 R)): the samples from a symbol's centre to the centre i symbols on (the sync's)."""
    R = int(rate)
    return (768000 * int(i) + R) // (2 * R)


class Settings:
    """What tfrec_amd_enable_burst_crc fixes; a ValueError where it returns E_INVAL."""

    def __init__(self, rate: int, n_bytes: int, width: int, poly: int, init: int = 0, xorout: int = 0, skip: int = 0,
                 lsb: bool = False, invert: bool = False):
        self.rate, self.N, self.W, self.S = int(rate), int(n_bytes), int(width), int(skip)
        self.poly, self.init, self.xorout, self.lsb, self.invert = int(poly), int(init), int(xorout), bool(lsb), bool(invert)
        if not 1000 <= self.rate <= 96000:
            raise ValueError("rate %d outside 1000 .. 96000" % self.rate)
        if not 1 <= self.N <= 256:
            raise ValueError("%d frame bytes outside 1 .. 256" % self.N)
        if self.W not in (8, 16, 24, 32):
            raise ValueError("width %d: one of 8, 16, 24, 32" % self.W)
        if self.S < 0 or self.S + self.W // 8 >= self.N:
            raise ValueError("skip %d: 0 <= skip and skip + width / 8 < n_bytes" % self.S)
        if self.poly == 0 or not all(0 <= x < 1 << self.W for x in (self.poly, self.init, self.xorout)):
            raise ValueError("poly non-zero; poly, init and xorout below 2^%d" % self.W)
        self.D = delta(self.rate, 8 * self.N)
        if self.D > HISTORY:
            raise ValueError("D %d above %d" % (self.D, HISTORY))
        self.offs = [self.D - delta(self.rate, i) for i in range(1, 8 * self.N + 1)]  # b_i is t[k - offs[i - 1]]
        self._table = None

    @property
    def flags(self) -> int:
        return (LSB if self.lsb else 0) | (INVERT if self.invert else 0)

    def args(self) -> tuple:
        """tfrec_amd_enable_burst_crc's arguments behind the context."""
        return (self.rate, self.N, self.S, self.W, self.poly, self.init, self.xorout, self.flags)

    def step8(self, r: int) -> int:
        """Eight shifts of the register."""
        for _ in range(8):
            r = ((r << 1) ^ self.poly if r >> (self.W - 1) & 1 else r << 1) & ((1 << self.W) - 1)
        return r

    def byte_of(self, bits8) -> int:
        """A byte from its eight bits in the order received."""
        return sum(int(b) << (q if self.lsb else 7 - q) for q, b in enumerate(bits8))

    def check(self, data) -> bool:
        """The header's CRC on a frame's N bytes: crc(covered) ^ xorout == field."""
        data = list(data)
        assert len(data) == self.N
        fb = self.W // 8
        r = self.init
        for x in data[self.S:self.N - fb]:
            r = self.step8(r ^ (int(x) << (self.W - 8)))
        return (r ^ self.xorout) == int.from_bytes(bytes(int(x) for x in data[self.N - fb:]), "big")

    def field_of(self, data) -> bytes:
        """The CRC field that makes the frame `data + field` check; data: its first N - W / 8 bytes."""
        r = self.init
        for x in list(data)[self.S:]:
            r = self.step8(r ^ (int(x) << (self.W - 8)))
        return (r ^ self.xorout).to_bytes(self.W // 8, "big")

    def _build(self):
        # The linear part, from the last covered byte back: a bit XORed into the register at bit W - 8 + p of byte j is shifted 8
        # times for its own byte and 8 times for every covered byte behind it.  A field bit contributes itself.
        fb = self.W // 8
        cols = [0] * (8 * self.N)
        unit = [self.step8(1 << (self.W - 8 + p)) for p in range(8)]  # by the bit's place in its byte
        for j in range(self.N - fb - 1, self.S - 1, -1):
            for q in range(8):
                cols[8 * j + q] = unit[q if self.lsb else 7 - q]
            # a byte further ahead: eight more shifts, which are linear
            unit = [self.step8(u) for u in unit]
        for j in range(self.N - fb, self.N):
            for q in range(8):
                cols[8 * j + q] = 1 << (8 * (self.N - 1 - j) + (q if self.lsb else 7 - q))
        r = self.init  # the constant: init through every covered byte of zeros, ^ xorout
        for _ in range(self.S, self.N - fb):
            r = self.step8(r)
        r0 = r ^ self.xorout
        if self.invert:  # every bit 1: all columns at once
            for c in cols:
                r0 ^= c
        self._table = [(o, c) for o, c in zip(self.offs, cols) if c]
        self._r0 = r0

    def table(self) -> list:
        """[(off_i, col_i)] for the i = 1 .. 8 N with col_i != 0, in the order of i."""
        if self._table is None:
            self._build()
        return self._table

    @property
    def r0(self) -> int:
        """The residue of the all-zero input track (INVERT folded in)."""
        if self._table is None:
            self._build()
        return self._r0


def fresh_state(n_streams: int) -> dict:
    """What a context carries before its first submit: no history."""
    return {"bits": [np.zeros(0, dtype=np.uint8) for _ in range(n_streams)]}


def _fits(rec, max_samples) -> bool:
    return max_samples is None or int(rec["bit_offset"]) + int(rec["n_samples"]) <= max_samples


def _copied(rec):
    o = np.zeros((), dtype=CRC_DTYPE)
    for f in ("stream", "flags", "start_sample", "n_samples", "thresh", "bit_offset"):
        o[f] = rec[f]
    o["first_at"] = NONE
    return o


def _history(rec, state):
    h = state["bits"][int(rec["stream"])] if int(rec["flags"]) & RUN_CONTINUES else np.zeros(0, dtype=np.uint8)
    return np.asarray(h, dtype=np.uint8)[-HISTORY:]


def _next_state(n_streams, trecs, tr, state, max_samples):
    """The state behind the submit: per stream the last 16383 input bits of the chain its OPEN run belongs to, as far as they were
    available to it; nothing behind a run that does not fit max_samples, and nothing without an OPEN run."""
    nxt = fresh_state(n_streams)
    for r, t in zip(trecs, tr):
        if int(r["flags"]) & RUN_OPEN and _fits(r, max_samples):
            nxt["bits"][int(r["stream"])] = np.concatenate([_history(r, state), t])[-HISTORY:]
    return nxt


def _tracks(trecs, twords, max_samples):
    return [track.bits_of(r, twords) if _fits(r, max_samples) else np.zeros(int(r["n_samples"]), dtype=np.uint8) for r in trecs]


def _begin(trecs, state, n_streams):
    if n_streams is None:
        n_streams = len(state["bits"]) if state is not None else int(max([int(r["stream"]) for r in trecs], default=-1)) + 1
    return n_streams, (fresh_state(n_streams) if state is None else state)


def _finish(o, v):
    ok = np.flatnonzero(v)
    o["n_ok"] = len(ok)
    o["first_at"] = int(ok[0]) if len(ok) else NONE


def crcs(trecs, twords, settings: Settings, state=None, n_streams=None, max_samples=None):
    """One submit.  trecs, twords: the submit's input records and bitmap (read_burst_codes' where the line code is on, else
    read_burst_tracks'; the records carry the table entry and its place in the pool); state: what the submit before returned
    (default: a fresh context's); n_streams: the context's (default: as many as the state or the records name); max_samples: the
    pool's size (default: everything fits) -> (a CRC_DTYPE array, one record per input record; the check bitmap's uint32 words,
    as many as the pairs that fit need; the state behind the submit)."""
    st = settings
    n_streams, state = _begin(trecs, state, n_streams)
    tr = _tracks(trecs, twords, max_samples)
    out = np.zeros(len(trecs), dtype=CRC_DTYPE)
    vs = []
    for e, (r, t) in enumerate(zip(trecs, tr)):
        o = _copied(r)
        n = len(t)
        v = np.zeros(n, dtype=np.uint8)
        if _fits(r, max_samples):
            h = _history(r, state)
            H = len(h)
            ext = np.concatenate([h, t]).astype(np.uint32)
            k0 = max(0, st.D - H)  # the first defined k
            if k0 < n:
                res = np.full(n - k0, st.r0, dtype=np.uint32)  # every plane at once: bit p of res is plane p
                for off, col in st.table():
                    a = H + k0 - off
                    res ^= ext[a:a + n - k0] * np.uint32(col)
                v[k0:] = res == 0
        _finish(o, v)
        out[e] = o
        vs.append(v)
    return out, track._pack(out, vs, max_samples), _next_state(n_streams, trecs, tr, state, max_samples)


def crcs_bruteforce(trecs, twords, settings: Settings, state=None, n_streams=None, max_samples=None):
    """The same, one sample at a time in Python integers, as the header words it: the bits b_i = t[k - (D - delta(i))] ^ invert,
    the bytes in the flag's order, the bitwise CRC over the covered ones, compared with the big-endian field."""
    st = settings
    n_streams, state = _begin(trecs, state, n_streams)
    tr = _tracks(trecs, twords, max_samples)
    out = np.zeros(len(trecs), dtype=CRC_DTYPE)
    vs = []
    inv = 1 if st.invert else 0
    fb = st.W // 8
    top, mask = 1 << (st.W - 1), (1 << st.W) - 1
    for e, (r, t) in enumerate(zip(trecs, tr)):
        o = _copied(r)
        tl = t.tolist()
        v = [0] * len(tl)
        if _fits(r, max_samples):
            h = _history(r, state).tolist()
            H = len(h)
            for k in range(len(tl)):
                if k + H < st.D:
                    continue
                b = []
                for i in range(1, 8 * st.N + 1):
                    x = k - (st.D - (768000 * i + st.rate) // (2 * st.rate))
                    b.append((tl[x] if x >= 0 else h[H + x]) ^ inv)
                data = []
                for j in range(st.N):
                    byte = 0
                    for q in range(8):
                        byte |= b[8 * j + q] << (q if st.lsb else 7 - q)
                    data.append(byte)
                reg = st.init
                for j in range(st.S, st.N - fb):
                    reg ^= data[j] << (st.W - 8)
                    for _ in range(8):
                        reg = ((reg << 1) ^ st.poly if reg & top else reg << 1) & mask
                field = 0
                for j in range(st.N - fb, st.N):
                    field = (field << 8) | data[j]
                v[k] = 1 if (reg ^ st.xorout) == field else 0
        v = np.array(v, dtype=np.uint8)
        _finish(o, v)
        out[e] = o
        vs.append(v)
    return out, track._pack(out, vs, max_samples), _next_state(n_streams, trecs, tr, state, max_samples)


bits_of = track.bits_of  # a record's check track out of its submit's bitmap -> uint8 [n_samples]


class Piece(track.Piece):
    """A check record with its check track."""


def merge(pieces):
    """A chain of pieces (in order, as for track.merge) -> one Piece, that of the uncut run: the check tracks concatenated,
    n_samples and n_ok added, first_at that of the first piece that has one, offset by the samples ahead of it; the flags as
    track.merge's."""
    pieces = list(pieces)
    o = pieces[0].rec.copy()
    for p in pieces[1:]:
        assert p["stream"] == o["stream"] and int(p["flags"]) & RUN_CONTINUES
        if int(o["first_at"]) == NONE and int(p["first_at"]) != NONE:
            o["first_at"] = int(o["n_samples"]) + int(p["first_at"])
        o["n_samples"] = int(o["n_samples"]) + int(p["n_samples"])
        o["n_ok"] = int(o["n_ok"]) + int(p["n_ok"])
    o["flags"] = (int(pieces[0]["flags"]) & RUN_CONTINUES) | (int(pieces[-1]["flags"]) & RUN_OPEN)
    return Piece(o, np.concatenate([p.bits for p in pieces]))


def chains(submits, restarts=None):
    """submits: one (records, words) per submit, in order -> the merged bursts as Pieces, in track.chains' order."""
    return burst.chains([[Piece(r, bits_of(r, w)) for r in recs] for recs, w in submits], restarts, join=merge)


def verdicts(frames, vpiece, settings: Settings) -> list:
    """The header's Verdict: sync.frames' frames of a chain (read with n_bytes = N) and the chain's merged check Piece -> per frame
    'ok' or 'bad' -- polarity + and all 8 N payload bits: v[c + D] -- or '-': no verdict."""
    st = settings
    out = []
    for c, _errors, pol, pay in frames:
        if pol != "+" or len(pay) != 8 * st.N:
            out.append("-")
        else:
            out.append("ok" if vpiece.bits[c + st.D] else "bad")
    return out


def line(name: str, vpiece, settings: Settings) -> str:
    """tfrec_gpu -V: crc <file> <start_sample> <n_samples> <n_ok> <sample|->: the last field is start_sample + first_at - D, where a
    sync word would have ended."""
    rec = vpiece.rec
    start, first = int(rec["start_sample"]), int(rec["first_at"])
    return "crc %s %d %d %d %s" % (name, start, int(rec["n_samples"]), int(rec["n_ok"]),
                                   "-" if first == NONE else str(start + first - settings.D))


def device_bytes(n_streams: int, max_runs: int, max_samples: int, n_bytes: int) -> int:
    """What tfrec_amd_enable_burst_crc adds to tfrec_amd_get_memory's device bytes: per FIFO set the records and the check bitmap;
    per stream the carried 512 words and H; once the term table, 8 N terms of 8 bytes."""
    from .api import FIFO_DEPTH
    return (FIFO_DEPTH * (max_runs * CRC_DTYPE.itemsize + 4 * ((max_samples + 31) // 32)) + n_streams * (4 * 512 + 4)
            + 8 * int(n_bytes) * 8)


def pinned_bytes(n_streams: int) -> int:
    """... and to its page-locked bytes: nothing."""
    return 0
