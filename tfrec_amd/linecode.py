"""The line code (tfrec_amd_enable_burst_code, include/tfrec_amd.h: "Line code") restated in numpy -- no GPU needed.
Written from the header's definition alone; exact integers throughout.

An optional stage of the burst track: per captured sample of every run of the recorder's table one bit, the track's bit XORed with
the track's bits delta(j) samples ahead of it for every set tap j -- a self-synchronising descrambler or a differential decoder on
the oversampled track --, complemented under INVERT, packed where the track's bit lies; per run a track record (TRACK_DTYPE) whose
n_ones is counted on the coded bits.  track.merge, track.slice_bits and sync.syncs / sync.frames work on the result unchanged.
Nothing here has been measured on real recordings.

  Settings           rate, taps and INVERT, checked as the enable call checks them;  named: g3ruh, nrzi, nrzs;
  codes              vectorised, from the definition: one submit's coded records and bitmap from the submit's track records and
                     track bitmap and the state the submit before left;
  codes_bruteforce   the same sample by sample, in Python integers;
  chains             the chains of a sequence of submits (track.chains on the result);
  device_bytes       what tfrec_amd_enable_burst_code adds to tfrec_amd_get_memory (pinned_bytes: nothing).
"""
from __future__ import annotations

import numpy as np

from . import track
from .capture import RUN_CONTINUES, RUN_OPEN
from .track import TRACK_DTYPE

HISTORY = 2047  # the track bits carried from submit to submit, and the largest span
INVERT = 1  # the flag: the coded bit is complemented
NAMED = {"g3ruh": (0x10800, False), "nrzi": (1, False), "nrzs": (1, True)}  # taps {12, 17}; {1}; {1} inverted


def delta(rate: int, j: int) -> int:
    """delta(j) = floor((768000 j + R) / (2 R)): the samples from a symbol's centre to the centre j symbols on (the sync's)."""
    R = int(rate)
    return (768000 * int(j) + R) // (2 * R)


class Settings:
    """What tfrec_amd_enable_burst_code fixes; a ValueError where it returns E_INVAL."""

    def __init__(self, rate: int, taps: int, invert: bool = False):
        self.rate, self.taps, self.invert = int(rate), int(taps), bool(invert)
        if not 1000 <= self.rate <= 96000:
            raise ValueError("rate %d outside 1000 .. 96000" % self.rate)
        if not 0 < self.taps < 1 << 32:
            raise ValueError("taps 0x%x: a non-zero uint32" % self.taps)
        self.delays = [j for j in range(1, 33) if (self.taps >> (j - 1)) & 1]  # in symbols
        self.delta = [delta(self.rate, j) for j in self.delays]  # in samples
        self.span = self.delta[-1]
        if self.span > HISTORY:
            raise ValueError("span %d above %d" % (self.span, HISTORY))

    @property
    def flags(self) -> int:
        return INVERT if self.invert else 0

    @classmethod
    def named(cls, name: str, rate: int):
        taps, inv = NAMED[name]
        return cls(rate, taps, inv)


def g3ruh(rate: int) -> Settings:
    return Settings.named("g3ruh", rate)


def nrzi(rate: int) -> Settings:
    return Settings.named("nrzi", rate)


def nrzs(rate: int) -> Settings:
    return Settings.named("nrzs", rate)


def fresh_state(n_streams: int) -> dict:
    """What a context carries before its first submit: no history."""
    return {"bits": [np.zeros(0, dtype=np.uint8) for _ in range(n_streams)]}


def _fits(rec, max_samples) -> bool:
    return max_samples is None or int(rec["bit_offset"]) + int(rec["n_samples"]) <= max_samples


def _history(rec, state):
    h = state["bits"][int(rec["stream"])] if int(rec["flags"]) & RUN_CONTINUES else np.zeros(0, dtype=np.uint8)
    return np.asarray(h, dtype=np.uint8)[-HISTORY:]


def _next_state(n_streams, trecs, tr, state, max_samples):
    """The state behind the submit: per stream the last 2047 TRACK bits of the chain its OPEN run belongs to, as far as they were
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


def codes(trecs, twords, settings: Settings, state=None, n_streams=None, max_samples=None):
    """One submit.  trecs, twords: the submit's track records and track bitmap (read_burst_tracks'); state: what the submit
    before returned (default: a fresh context's); n_streams: the context's (default: as many as the state or the records name);
    max_samples: the pool's size (default: everything fits) -> (a TRACK_DTYPE array, one record per track record: the track
    record with n_ones counted on the coded bits; the coded bitmap's uint32 words, as many as the pairs that fit need; the state
    behind the submit)."""
    st = settings
    n_streams, state = _begin(trecs, state, n_streams)
    tr = _tracks(trecs, twords, max_samples)
    out = np.array(trecs, dtype=TRACK_DTYPE).copy().reshape(-1)
    us = []
    for e, (r, t) in enumerate(zip(trecs, tr)):
        n = len(t)
        u = np.zeros(n, dtype=np.uint8)
        if _fits(r, max_samples):
            ext = np.concatenate([np.zeros(st.span, dtype=np.uint8), _history(r, state), t])  # (ahead of the chain: 0)
            z = len(ext) - n  # ext[z + k] = t[k]
            u = t.copy()
            for d in st.delta:
                u ^= ext[z - d:z - d + n]
            if st.invert:
                u ^= 1
        out[e]["n_ones"] = int(np.count_nonzero(u))
        us.append(u)
    return out, track._pack(out, us, max_samples), _next_state(n_streams, trecs, tr, state, max_samples)


def codes_bruteforce(trecs, twords, settings: Settings, state=None, n_streams=None, max_samples=None):
    """The same, one sample at a time in Python integers, as the header words it: u[k] = t[k] ^ XOR over the taps of
    t[k - delta(j)] ^ invert, t[x] = 0 ahead of the H available bits."""
    st = settings
    n_streams, state = _begin(trecs, state, n_streams)
    tr = _tracks(trecs, twords, max_samples)
    out = np.array(trecs, dtype=TRACK_DTYPE).copy().reshape(-1)
    us = []
    for e, (r, t) in enumerate(zip(trecs, tr)):
        tl = t.tolist()
        u = [0] * len(tl)
        if _fits(r, max_samples):
            h = _history(r, state).tolist()
            H = len(h)

            def bit(x):  # t[x]
                return tl[x] if x >= 0 else h[H + x] if x >= -H else 0

            for k in range(len(tl)):
                v = bit(k) ^ (1 if st.invert else 0)
                for j in st.delays:
                    v ^= bit(k - (768000 * j + st.rate) // (2 * st.rate))
                u[k] = v
        out[e]["n_ones"] = sum(u)
        us.append(np.array(u, dtype=np.uint8))
    return out, track._pack(out, us, max_samples), _next_state(n_streams, trecs, tr, state, max_samples)


def chains(submits, restarts=None):
    """submits: one (coded records, coded words) per submit, in order -> the merged bursts as track.Pieces, in track.chains' order."""
    return track.chains(submits, restarts)


def line(name: str, piece, rate: int) -> str:
    """tfrec_gpu -U: code <file> <start_sample> <n_samples> <burst_samples> <n_bits>[+] <hex|->: track.line's slice of the coded track."""
    return "code" + track.line(name, piece, rate)[4:]


def device_bytes(n_streams: int, max_runs: int, max_samples: int) -> int:
    """What tfrec_amd_enable_burst_code adds to tfrec_amd_get_memory's device bytes: per FIFO set the records and the coded
    bitmap; per stream the carried 64 words and H."""
    from .api import FIFO_DEPTH
    return FIFO_DEPTH * (max_runs * TRACK_DTYPE.itemsize + 4 * ((max_samples + 31) // 32)) + n_streams * (4 * 64 + 4)


def pinned_bytes(n_streams: int) -> int:
    """... and to its page-locked bytes: nothing."""
    return 0
