"""The packet check (tfrec_amd_enable_burst_packets, include/tfrec_amd.h: "Packet check") restated in Python integers
-- no GPU needed.  Written from the header's definition alone: one candidate at a time, bytes assembled one by one, a bitwise CRC.

An optional stage behind the burst sync: every set bit c of the sync's match track is a candidate packet -- a length byte L behind
the sync word, T = 1 + L + len_add + W / 8 bytes in all, de-whitened, ending at k = c + delta(8 T) --, and per captured sample one
bit says whether a candidate that ends there carries its own CRC; per run a 48-byte record.  Nothing here has been measured on real
recordings.

  Settings           what the enable call fixes, checked as it checks them (sync: the sync's settings, for the refusals that need them);
  pn9                the CC1101's whitening sequence;
  packets            one submit's records and ok bitmap from the submit's input records and bitmap (the sync's input), the
                     sync's records and match bitmap, and the state the submit before left;
  bits_of            a record's ok track out of the bitmap;  merge: a chain of pieces -> the record and ok track of the uncut
                     run;  chains: the chains of a sequence of submits (burst.chains' walk);
  read               a chain's merged input track, match track and ok track -> per plateau (c, L, 'ok' | 'bad' | '-', bytes);
  line, summary_line a host program's lines per plateau and per burst;
  device_bytes       what tfrec_amd_enable_burst_packets adds to tfrec_amd_get_memory (pinned_bytes: nothing).
"""
from __future__ import annotations

import numpy as np

from . import burst, sync, track
from .capture import RUN_CONTINUES, RUN_OPEN
from .crc import HISTORY, INVERT, LSB, NONE, delta

MAX_WHITEN, MAX_ADD = 274, 16
PACKET_DTYPE = np.dtype([("stream", "<u4"), ("flags", "<u4"), ("start_sample", "<i8"), ("n_samples", "<u4"), ("thresh", "<i4"),
                         ("bit_offset", "<u8"), ("n_seen", "<u4"), ("n_ok", "<u4"), ("first_at", "<u4"), ("reserved", "<u4")])
assert PACKET_DTYPE.itemsize == 48


def pn9(n: int) -> bytes:
    """The CC1101's PN9 sequence: a 9-bit register seeded 0x1FF; a byte is its low 8 bits, then eight steps of new = b0 ^ b5, shift
    right, new into bit 8."""
    r, out = 0x1FF, []
    for _ in range(int(n)):
        out.append(r & 0xFF)
        for _ in range(8):
            r = (r >> 1) | (((r ^ (r >> 5)) & 1) << 8)
    return bytes(out)


class Settings:
    """What tfrec_amd_enable_burst_packets fixes; a ValueError where it returns E_INVAL.  sync: the context's sync.Settings (None:
    no sync is enabled, which is refused)."""

    def __init__(self, rate: int, len_max: int, width: int, poly: int, init: int = 0, xorout: int = 0, len_min: int = 0, len_add: int = 0,
                 skip: int = 0, whiten: bytes = b"", lsb: bool = False, invert: bool = False, sync=Ellipsis):
        self.rate, self.len_min, self.len_max, self.add, self.S, self.W = int(rate), int(len_min), int(len_max), int(len_add), int(skip), int(width)
        self.poly, self.init, self.xorout, self.lsb, self.invert = int(poly), int(init), int(xorout), bool(lsb), bool(invert)
        self.whiten = bytes(whiten)
        if sync is None:
            raise ValueError("the packet check works on the burst sync's matches")
        if sync is not Ellipsis and (sync.rate != self.rate or sync.both):
            raise ValueError("the sync's rate is %d and its BOTH %s" % (sync.rate, sync.both))
        if not 1000 <= self.rate <= 96000:
            raise ValueError("rate %d outside 1000 .. 96000" % self.rate)
        if not 0 <= self.len_min <= self.len_max <= 255:
            raise ValueError("lengths %d .. %d: 0 <= len_min <= len_max <= 255" % (self.len_min, self.len_max))
        if not 0 <= self.add <= MAX_ADD:
            raise ValueError("len_add %d outside 0 .. 16" % self.add)
        if self.W not in (8, 16, 24, 32):
            raise ValueError("width %d: one of 8, 16, 24, 32" % self.W)
        if not 0 <= self.S < 1 + self.len_min + self.add:
            raise ValueError("skip %d: 0 <= skip < 1 + len_min + len_add, so that a byte is covered" % self.S)
        if self.poly == 0 or not all(0 <= x < 1 << self.W for x in (self.poly, self.init, self.xorout)):
            raise ValueError("poly non-zero; poly, init and xorout below 2^%d" % self.W)
        if len(self.whiten) > MAX_WHITEN:
            raise ValueError("%d whitening bytes above %d" % (len(self.whiten), MAX_WHITEN))
        self.reach = delta(self.rate, 8 * self.total(self.len_max))
        if self.reach > HISTORY:
            raise ValueError("the longest packet reaches %d samples, above %d" % (self.reach, HISTORY))

    @property
    def flags(self) -> int:
        return (LSB if self.lsb else 0) | (INVERT if self.invert else 0)

    def args(self) -> dict:
        """api.Receiver.enable_burst_packets' arguments."""
        return dict(rate=self.rate, len_max=self.len_max, width=self.W, poly=self.poly, init=self.init, xorout=self.xorout, len_min=self.len_min,
                    len_add=self.add, skip=self.S, whiten=self.whiten, lsb=self.lsb, invert=self.invert)

    def total(self, L: int) -> int:
        """T: the length byte, the L bytes it counts, len_add more and the CRC field."""
        return 1 + int(L) + self.add + self.W // 8

    def byte(self, bit, c: int, j: int) -> int:
        """Byte j of the candidate at c, de-whitened; bit(k): the chain's input bit at k."""
        v = 0
        for q in range(8):
            b = int(bit(c + delta(self.rate, 8 * j + q + 1))) ^ (1 if self.invert else 0)
            v |= b << (q if self.lsb else 7 - q)
        return v ^ (self.whiten[j] if j < len(self.whiten) else 0)

    def crc(self, data) -> int:
        """The header's CRC over bytes: unreflected, bit by bit."""
        r, top, mask = self.init, 1 << (self.W - 1), (1 << self.W) - 1
        for x in data:
            r ^= int(x) << (self.W - 8)
            for _ in range(8):
                r = ((r << 1) ^ self.poly if r & top else r << 1) & mask
        return r ^ self.xorout

    def check(self, data) -> bool:
        """A packet's T de-whitened bytes: the CRC over bytes skip .. T - W / 8 - 1 equals the big-endian field."""
        data, fb = list(data), self.W // 8
        return self.crc(data[self.S:len(data) - fb]) == int.from_bytes(bytes(data[len(data) - fb:]), "big")

    def packet_of(self, payload) -> bytes:
        """The de-whitened bytes of a packet that checks: the length byte (which counts the payload less len_add), the payload and
        the field."""
        payload = bytes(payload)
        data = bytes([len(payload) - self.add]) + payload
        return data + self.crc(data[self.S:]).to_bytes(self.W // 8, "big")

    def on_air(self, data) -> list:
        """De-whitened bytes -> the bits as they stand on the input track, in the order received."""
        inv = 1 if self.invert else 0
        raw = [x ^ (self.whiten[j] if j < len(self.whiten) else 0) for j, x in enumerate(data)]
        return [((x >> (q if self.lsb else 7 - q)) & 1) ^ inv for x in raw for q in range(8)]


def fresh_state(n_streams: int) -> dict:
    """What a context carries before its first submit: no history.  bits: the input's; match: the sync's, as long."""
    z = lambda: [np.zeros(0, dtype=np.uint8) for _ in range(n_streams)]  # noqa: E731
    return {"bits": z(), "match": z()}


def _fits(rec, max_samples) -> bool:
    return max_samples is None or int(rec["bit_offset"]) + int(rec["n_samples"]) <= max_samples


def packets(xrecs, xwords, mrecs, mwords, settings: Settings, state=None, n_streams=None, max_samples=None):
    """One submit.  xrecs, xwords: the submit's input records and bitmap (read_burst_codes' where the line code is on, else
    read_burst_tracks'); mrecs, mwords: read_burst_syncs' of the same submit; state: what the submit before returned -> (a
    PACKET_DTYPE array, one record per input record; the ok bitmap's uint32 words; the state behind the submit)."""
    st = settings
    if n_streams is None:
        n_streams = len(state["bits"]) if state is not None else int(max([int(r["stream"]) for r in xrecs], default=-1)) + 1
    state = fresh_state(n_streams) if state is None else state
    nxt = fresh_state(n_streams)
    out = np.zeros(len(xrecs), dtype=PACKET_DTYPE)
    vs = []
    for e, (r, mr) in enumerate(zip(xrecs, mrecs)):
        o = out[e]
        for f in ("stream", "flags", "start_sample", "n_samples", "thresh", "bit_offset"):
            o[f] = r[f]
        o["first_at"] = NONE
        n, s = int(r["n_samples"]), int(r["stream"])
        v = np.zeros(n, dtype=np.uint8)
        if _fits(r, max_samples):
            cont = int(r["flags"]) & RUN_CONTINUES
            hx = (state["bits"][s] if cont else np.zeros(0, dtype=np.uint8))[-HISTORY:].tolist()
            hm = (state["match"][s] if cont else np.zeros(0, dtype=np.uint8))[-HISTORY:].tolist()
            H = len(hx)
            x, m = hx + track.bits_of(r, xwords).tolist(), hm + sync.bits_of(mr, mwords).tolist()
            seen = ok = 0
            for c in range(-H, n):  # the chain holds everything from c on
                if not m[H + c]:
                    continue
                if c + delta(st.rate, 8) >= n:
                    continue  # not even the length byte: the end lies behind the piece
                L = st.byte(lambda k: x[H + k], c, 0)
                if not st.len_min <= L <= st.len_max:
                    continue
                T = st.total(L)
                k = c + delta(st.rate, 8 * T)
                if not 0 <= k < n:
                    continue  # evaluated by the piece that holds k, if there is one
                seen += 1
                if st.check([st.byte(lambda i: x[H + i], c, j) for j in range(T)]):
                    ok += 1
                    v[k] = 1
                    o["first_at"] = min(int(o["first_at"]), k)
            o["n_seen"], o["n_ok"] = seen, ok
            if int(r["flags"]) & RUN_OPEN:
                nxt["bits"][s] = np.array(x[-HISTORY:], dtype=np.uint8)
                nxt["match"][s] = np.array(m[-HISTORY:], dtype=np.uint8)
        vs.append(v)
    return out, track._pack(out, vs, max_samples), nxt


bits_of = track.bits_of  # a record's ok track out of its submit's bitmap -> uint8 [n_samples]


class Piece(track.Piece):
    """A packet record with its ok track."""


def merge(pieces):
    """A chain of pieces (in order, as for track.merge) -> one Piece, that of the uncut run: the ok tracks concatenated, n_samples,
    n_seen and n_ok added, first_at that of the first piece that has one, offset by the samples ahead of it."""
    pieces = list(pieces)
    o = pieces[0].rec.copy()
    for p in pieces[1:]:
        assert p["stream"] == o["stream"] and int(p["flags"]) & RUN_CONTINUES
        if int(o["first_at"]) == NONE and int(p["first_at"]) != NONE:
            o["first_at"] = int(o["n_samples"]) + int(p["first_at"])
        o["n_samples"] = int(o["n_samples"]) + int(p["n_samples"])
        o["n_seen"] = int(o["n_seen"]) + int(p["n_seen"])
        o["n_ok"] = int(o["n_ok"]) + int(p["n_ok"])
    o["flags"] = (int(pieces[0]["flags"]) & RUN_CONTINUES) | (int(pieces[-1]["flags"]) & RUN_OPEN)
    return Piece(o, np.concatenate([p.bits for p in pieces]))


def chains(submits, restarts=None):
    """submits: one (records, words) per submit, in order -> the merged bursts as Pieces, in track.chains' order."""
    return burst.chains([[Piece(r, bits_of(r, w)) for r in recs] for recs, w in submits], restarts, join=merge)


def read(tpiece, spiece, vpiece, settings: Settings) -> list:
    """A chain's merged input track (a track.Piece), match track and ok track -> for each of sync.plateaus' centres c inside the
    burst (c, L, 'ok' | 'bad' | '-', the packet's de-whitened bytes): '-' (and L None or no bytes) where the length byte or the
    packet's end lies behind the burst, or L is out of range; else the ok track's bit at the packet's end."""
    st = settings
    length = min(int(tpiece.rec["last_over"]) + 1, sync.KEEP, len(tpiece.bits))
    t = tpiece.bits[:length].tolist()
    out = []
    for a, b in sync.plateaus(spiece.bits[:length]):
        c = (a + b) >> 1
        if c + delta(st.rate, 8) >= length:
            out.append((c, None, "-", b""))
            continue
        L = st.byte(t.__getitem__, c, 0)
        k = c + delta(st.rate, 8 * st.total(L))
        if not st.len_min <= L <= st.len_max or k >= length:
            out.append((c, L, "-", b""))
            continue
        data = bytes(st.byte(t.__getitem__, c, j) for j in range(st.total(L)))
        out.append((c, L, "ok" if vpiece.bits[k] else "bad", data))
    return out


def line(name: str, vpiece, item) -> str:
    """A plateau's line: packet <file> <start_sample> <sync_sample> <len|-> <ok|bad|-> <hex|->."""
    c, L, verdict, data = item
    start = int(vpiece.rec["start_sample"])
    return "packet %s %d %d %s %s %s" % (name, start, start + c, "-" if L is None else L, verdict, data.hex() if data else "-")


def summary_line(name: str, vpiece) -> str:
    """A burst's line: pkts <file> <start_sample> <n_samples> <n_seen> <n_ok> <sample|->: the last field is start_sample + first_at,
    where the first packet that checks ends."""
    rec = vpiece.rec
    start, first = int(rec["start_sample"]), int(rec["first_at"])
    return "pkts %s %d %d %d %d %s" % (name, start, int(rec["n_samples"]), int(rec["n_seen"]), int(rec["n_ok"]),
                                       "-" if first == NONE else str(start + first))


def device_bytes(n_streams: int, max_runs: int, max_samples: int) -> int:
    """What tfrec_amd_enable_burst_packets adds to tfrec_amd_get_memory's device bytes: per FIFO set the records and the ok
    bitmap; per stream the carried 1024 words and H; once the tables, 3 x 276 words."""
    from .api import FIFO_DEPTH
    return FIFO_DEPTH * (max_runs * PACKET_DTYPE.itemsize + 4 * ((max_samples + 31) // 32)) + n_streams * (4 * 1024 + 4) + 4 * 3 * 276


def pinned_bytes(n_streams: int) -> int:
    """... and to its page-locked bytes: nothing."""
    return 0
